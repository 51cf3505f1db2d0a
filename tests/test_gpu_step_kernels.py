"""The code that runs every training step around the convs: the graph-replayed
solver step, the multi-tensor update / zero / repack / unpack / colsum kernels
and the single-tensor optimizers.

Every reference is computed here, in fp64 or integer arithmetic, from the
f32 / bf16 values the kernel reads (section A compares with eager training,
which is the reference the graphed step has to reproduce). Outputs live
inside sentinel-filled backing buffers that are compared whole, so a write
outside a tensor fails the comparison too."""

import functools

import pytest
import torch

import poseidon_amd as pa
from poseidon_amd.ops import functional as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24          # unit roundoff of f32 (round to nearest)
MT_CHUNK = 8192         # ps_mt.h
SENTINEL = 7777.0


def _f32(v):
    """A python scalar as the bindings pass it on: rounded to f32."""
    return float(torch.tensor(float(v), dtype=torch.float32).item())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class Arena:
    """Tensors carved out of one 1-D backing buffer: each starts at a multiple
    of 64 elements and has at least 64 sentinel elements on either side."""

    def __init__(self, sizes):
        self.sizes = list(sizes)
        self.starts = []
        off = 64
        for n in self.sizes:
            self.starts.append(off)
            off = (off + n + 64 + 63) // 64 * 64
        self.total = off

    def slices(self):
        return [slice(s, s + n) for s, n in zip(self.starts, self.sizes)]

    def new(self, dtype=torch.float32, fill=SENTINEL):
        return torch.full((self.total,), fill, dtype=dtype)

    def views(self, buf):
        return [buf.narrow(0, s, n) for s, n in zip(self.starts, self.sizes)]


def _worst(err, bound):
    """Largest err / bound, for the assertion message (huge where a
    sentinel, whose bound is 0, was overwritten)."""
    return (err / bound.clamp(min=1e-300)).max().item()


def _check_within(got, ref, bound, what):
    """|got - ref| <= bound element-wise over a whole backing buffer; the
    bound is 0 outside the tensors, where the sentinels must be intact."""
    err = (got.detach().cpu().double() - ref).abs()
    worst = _worst(err, bound)
    print(f"{what}: max err {err.max().item():.3e}, worst err/bound "
          f"{worst:.3f}")
    assert bool((err <= bound).all()), \
        f"{what}: {int((err > bound).sum())} elements over the bound, " \
        f"worst err/bound {worst:.3f} at {int((err - bound).argmax())}"


# ---------------------------------------------------------------------------
# A. graphed training equals eager training
# ---------------------------------------------------------------------------

_STEP_NET = """
    name: "stepnet"
    layers { name: "data" type: DUMMY_DATA top: "data" top: "label"
             dummy_data_param { num: 4 channels: 3 height: 8 width: 8
                 num: 4 channels: 1 height: 1 width: 1
                 data_filler { type: "gaussian" std: 1.0 }
                 data_filler { type: "constant" } } }
    layers { name: "c1" type: CONVOLUTION bottom: "data" top: "c1"
             blobs_lr: 1 blobs_lr: 2 weight_decay: 1 weight_decay: 0
             convolution_param { num_output: 8 kernel_size: 3 pad: 1
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "r1" type: RELU bottom: "c1" top: "c1" }
    layers { name: "p1" type: POOLING bottom: "c1" top: "p1"
             pooling_param { pool: MAX kernel_size: 2 stride: 2 } }
    layers { name: "ip" type: INNER_PRODUCT bottom: "p1" top: "ip"
             inner_product_param { num_output: 5
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" } } }
    layers { name: "loss" type: SOFTMAX_LOSS bottom: "ip" bottom: "label"
             top: "loss" }
"""

# Worst element-wise difference of any owned parameter or history tensor
# between two eager runs of _train with the same seed and data, over three
# pairs of runs per compute dtype, measured on an MI355X: 2.980e-08,
# 3.725e-08 and 2.980e-08 in fp32 (one to one and a half ulps of the largest
# weights; some f32 kernel accumulates in an order that varies). bf16
# training repeated bit for bit in all three pairs. A second set of three
# pairs, taken after the solver fix, gave 4.470e-08 / 1.490e-08 / 4.470e-08
# and 0 again; the constant stays at the first set's figure. Graphed against
# eager at that time: 2.980e-08 and 5.960e-08 in fp32, 0 in bf16.
D0 = {"fp32": 3.725e-08, "bf16": 0.0}


def _train(dtype, graphed):
    """step(5) then step(3) of the step net; returns (iter, params, history)
    of the owned parameters, on the CPU."""
    from poseidon_amd.proto import Message, parse_text
    from poseidon_amd.solver.solver import SGDSolver

    pa.init(device="cuda", seed=1234, compute_dtype=dtype)
    try:
        sp = Message("SolverParameter", base_lr=0.05, lr_policy="step",
                     stepsize=2, gamma=0.5, momentum=0.9, weight_decay=0.001,
                     max_iter=100, display=0, snapshot=0)
        sp.net_param = parse_text("NetParameter", _STEP_NET)
        s = SGDSolver(sp, verbose=False)
        g = _gen(17)
        data = torch.randn(4, 3, 8, 8, generator=g).to(torch.bfloat16).float()
        labels = torch.tensor([0.0, 2.0, 4.0, 1.0]).view(4, 1, 1, 1)
        s.net.blobs["data"].data = data.to(DEV, dtype)
        s.net.blobs["label"].data = labels.to(DEV)
        s.net.layers[0]._filled = True
        s.net.layers[0].refill = [False, False]
        if graphed:
            assert s.enable_graph() is True
        s.step(5)
        s.step(3)
        torch.cuda.synchronize()
        if graphed:
            # a capture that failed falls back to eager and clears these
            assert s._use_graph and s._graph is not None
        owned = [i for i, ps in enumerate(s.net.params) if ps.owner == i]
        assert sorted(s.history) == owned and len(owned) == 4
        return (s.iter,
                [s.net.params[i].blob.data.detach().cpu().clone()
                 for i in owned],
                [s.history[i].detach().cpu().clone() for i in owned])
    finally:
        pa.init(device="cpu", compute_dtype=torch.float32)


def _state_diff(a, b):
    """Worst element-wise difference of the parameters and history."""
    return max((x.double() - y.double()).abs().max().item()
               for ta, tb in zip(a[1:], b[1:]) for x, y in zip(ta, tb))


def _ulp32(x):
    a = x.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_graphed_training_equals_eager(name):
    """After enable_graph(), step(n) leaves the solver where eager step(n)
    leaves it: iter, every owned parameter, every history tensor. The lr
    policy halves the rate every two iterations, so it changes within the
    capture's warm-up passes and again between replays (the replayed
    sgd_mt kernel must read it from device memory each time). Bound: 4 * D0
    (the run-to-run difference of eager training, the reference), and no
    less than one f32 ulp of the compared value.

    Before SGDSolver._capture_graph restored the parameters and history its
    three warm-up passes change, the warm-ups were three uncounted updates
    and graphed training ended 1.7e-01 (parameters) and 6.6e-03 (history)
    away from eager training in both compute dtypes.

    Not covered: layers with device-side per-iteration state (dropout's
    offset counter advances during the warm-up passes)."""
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[name]
    eager = _train(dtype, graphed=False)
    again = _train(dtype, graphed=False)
    graph = _train(dtype, graphed=True)
    print(f"{name}: eager-eager {_state_diff(eager, again):.3e} "
          f"(D0 {D0[name]:.3e}), graphed-eager "
          f"{_state_diff(eager, graph):.3e}")
    assert eager[0] == 8 and graph[0] == 8
    for kind, ts_g, ts_e in (("param", graph[1], eager[1]),
                             ("history", graph[2], eager[2])):
        for k, (tg, te) in enumerate(zip(ts_g, ts_e)):
            err = (tg.double() - te.double()).abs()
            bound = _ulp32(te).clamp(min=4.0 * D0[name])
            assert bool((err <= bound).all()), \
                f"{name} {kind} {k}: max |graphed - eager| " \
                f"{err.max().item():.3e}, bound {bound.min().item():.3e}"


# ---------------------------------------------------------------------------
# B. sgd_mt and zero_mt
# ---------------------------------------------------------------------------

# one element, a scalar tail, vec4 + tail, one under / exactly / one over a
# chunk, two chunks + a 5-element tail (vec4 + scalar), several chunks
MT_LENGTHS = [1, 3, 5, MT_CHUNK - 1, MT_CHUNK, MT_CHUNK + 1, 16389, 40000]
MT_LR_MULT = [1.0, 2.0, 0.5, 1.5, 0.25, 3.0, 1.0, 0.75]
MT_WD = [0.0, 5e-4, 1e-3, 2e-3, 0.0, 1e-4, 5e-3, 1e-2]


def _sgd_reference(W, G, H, slices, lr, lr_mults, mom, wds):
    """fp64 h' = mom h + lr lr_mult (g + wd w), w' = w - h' over whole
    backing buffers (untouched outside the tensors), and the bound.

    Bound 8 u (|mom h| + |lr g| + |lr wd w| + |w|), u = 2^-24: the kernel
    rounds wd*w, g + that, lr*lr_mult, the product of the two, mom*h and
    their sum -- at most five roundings on any term of h', each relative to
    a partial result no larger than S = |mom h| + |lr g| + |lr wd w|, so
    |dh| <= 5 u S (an FMA contraction only removes a rounding). w' = w - h'
    adds one rounding of at most u (|w| + S): |dw| <= 6 u S + u |w|. 8 u
    (S + |w|) covers both with the second-order terms."""
    Wr, Hr = W.double().clone(), H.double().clone()
    B = torch.zeros_like(Wr)
    mom = _f32(mom)
    for sl, lm, wd in zip(slices, lr_mults, wds):
        w, g, h = W[sl].double(), G[sl].double(), H[sl].double()
        lrt, wd = _f32(lr) * _f32(lm), _f32(wd)
        Hr[sl] = mom * h + lrt * (g + wd * w)
        Wr[sl] = w - Hr[sl]
        B[sl] = 8 * U * ((mom * h).abs() + (lrt * g).abs()
                         + (lrt * wd * w).abs() + w.abs())
    return Wr, Hr, B


@pytest.mark.parametrize("use_lr_dev", [False, True], ids=["lr", "lr_dev"])
def test_sgd_mt(use_lr_dev):
    arena = Arena(MT_LENGTHS)
    sl = arena.slices()
    W, G, H = arena.new(), arena.new(), arena.new()
    for k, s in enumerate(sl):
        n = s.stop - s.start
        W[s] = torch.randn(n, generator=_gen(100 + k))
        G[s] = torch.randn(n, generator=_gen(200 + k))
        H[s] = torch.randn(n, generator=_gen(300 + k)) * 0.1
    Wd, Gd, Hd = W.to(DEV), G.to(DEV), H.to(DEV)
    mt = ops.sgd_mt_prepare(arena.views(Wd), arena.views(Gd), arena.views(Hd),
                            MT_LR_MULT, MT_WD)
    assert mt[2] == sum((n + MT_CHUNK - 1) // MT_CHUNK for n in MT_LENGTHS)
    lr, mom = 0.03, 0.9
    # with lr_dev the rate comes from device memory: a kernel that took the
    # scalar instead would be off by a factor of 20
    lr_dev = (torch.full((1,), lr, dtype=torch.float32, device=DEV)
              if use_lr_dev else None)
    for step in range(2):
        # the second step starts from what the kernel left: history carries
        Wr, Hr, B = _sgd_reference(W, G, H, sl, lr, MT_LR_MULT, mom, MT_WD)
        ops.sgd_mt_run(mt, 0.6 if use_lr_dev else lr, mom, lr_dev)
        torch.cuda.synchronize()
        _check_within(Wd, Wr, B, f"sgd_mt step {step} w")
        _check_within(Hd, Hr, B, f"sgd_mt step {step} h")
        assert torch.equal(Gd.cpu(), G), "sgd_mt wrote the gradients"
        W, H = Wd.cpu(), Hd.cpu()


def test_zero_mt():
    arena = Arena(MT_LENGTHS)
    P = arena.new()
    for k, s in enumerate(arena.slices()):
        P[s] = torch.randn(s.stop - s.start, generator=_gen(400 + k)) + 3.0
    Pd = P.to(DEV)
    mt = ops.zero_mt_prepare(arena.views(Pd))
    ops.zero_mt_run(mt)
    torch.cuda.synchronize()
    want = arena.new()
    for s in arena.slices():
        want[s] = 0.0
    assert torch.equal(Pd.cpu(), want)


# ---------------------------------------------------------------------------
# C. single-tensor optimizers
# ---------------------------------------------------------------------------

def _one_tensor(n, seed, h_abs=False):
    """w, g, h of length n, each inside its own guarded backing buffer."""
    arena = Arena([n])
    s = arena.slices()[0]
    bufs = []
    for k in range(3):
        b = arena.new()
        b[s] = torch.randn(n, generator=_gen(seed + k))
        bufs.append(b)
    if h_abs:
        bufs[2][s] = bufs[2][s].abs() + 1e-3
    else:
        bufs[2][s] *= 0.1
    return arena, s, bufs


# 2097157 > 2048 * 256 * 4: the vec4 body takes a second grid-stride pass,
# and 2097157 % 4 = 1 runs the tail kernel; 1 and 3 run the tail alone
@pytest.mark.parametrize("use_lr_dev", [False, True], ids=["lr", "lr_dev"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1027, 2097157])
def test_sgd_update(n, use_lr_dev):
    """Bound: _sgd_reference's (with lr_dev the kernel rounds lr_dev *
    lr_mult, without it the rate arrives rounded once: no more roundings
    than the multi-tensor kernel either way)."""
    arena, s, (W, G, H) = _one_tensor(n, seed=500)
    Wd, Gd, Hd = W.to(DEV), G.to(DEV), H.to(DEV)
    w, g, h = (arena.views(t)[0] for t in (Wd, Gd, Hd))
    mom, wd = 0.9, 1e-3
    if use_lr_dev:
        lr, lr_mult = 0.03, 2.0
        lr_dev = torch.full((1,), lr, dtype=torch.float32, device=DEV)
        ops.sgd_update(w, g, h, lr_mult, mom, wd, lr_dev=lr_dev)
    else:
        lr, lr_mult = 0.06, 1.0
        ops.sgd_update(w, g, h, lr, mom, wd)
    torch.cuda.synchronize()
    Wr, Hr, B = _sgd_reference(W, G, H, [s], lr, [lr_mult], mom, [wd])
    _check_within(Wd, Wr, B, f"sgd_update n={n} w")
    _check_within(Hd, Hr, B, f"sgd_update n={n} h")
    assert torch.equal(Gd.cpu(), G)


def test_nesterov_update():
    """n = 524291 > 2048 * 256: three elements take a second grid-stride
    pass. h' = mom h + lr (g + wd w); w' = w - ((1 + mom) h' - mom h).

    Bounds, u = 2^-24, S = |mom h| + |lr g| + |lr wd w| >= |h'|:
    h' as in _sgd_reference less the lr*lr_mult product: |dh| <= 4 u S; the
    test allows 6 u S. The update rounds 1 + mom and its product with h'
    (2 u (1+mom) S, on top of (1+mom) |dh|), mom*h (u S), the difference
    (u ((1+mom) S + S)) and w - update (u (|w| + (1+mom) S + S)): in all
    u (9 (1+mom) S + 3 S + |w|) to first order with |dh| <= 5 u S; the test
    allows u (12 (1+mom) S + 2 |w|), which is no smaller."""
    n = 524291
    arena, s, (W, G, H) = _one_tensor(n, seed=600)
    Wd, Gd, Hd = W.to(DEV), G.to(DEV), H.to(DEV)
    lr, mom, wd = 0.1, 0.9, 1e-3
    ops.nesterov_update(*(arena.views(t)[0] for t in (Wd, Gd, Hd)),
                        lr, mom, wd)
    torch.cuda.synchronize()
    lr, mom, wd = _f32(lr), _f32(mom), _f32(wd)
    w, g, h = W[s].double(), G[s].double(), H[s].double()
    Wr, Hr = W.double().clone(), H.double().clone()
    Bw, Bh = torch.zeros_like(Wr), torch.zeros_like(Wr)
    Hr[s] = mom * h + lr * (g + wd * w)
    Wr[s] = w - ((1.0 + mom) * Hr[s] - mom * h)
    S = (mom * h).abs() + (lr * g).abs() + (lr * wd * w).abs()
    Bh[s] = 6 * U * S
    Bw[s] = U * (12 * (1.0 + mom) * S + 2 * w.abs())
    _check_within(Wd, Wr, Bw, "nesterov w")
    _check_within(Hd, Hr, Bh, "nesterov h")
    assert torch.equal(Gd.cpu(), G)


def test_adagrad_update():
    """n = 524291 > 2048 * 256. gv = g + wd w; h' = h + gv^2;
    w' = w - lr gv / (sqrt(h') + delta), with h >= 1e-3.

    Bounds to first order, u = 2^-24 (sqrtf and the f32 divide round
    correctly):
      gv  two roundings:            dg <= 2 u Sg,  Sg = |g| + |wd w|
      h'  gv^2 and the sum round:   dh <= 2 |gv| dg + u gv^2 + u (h + gv^2)
      q = lr gv / D, D = sqrt(h') + delta:
          from gv                   lr dg / D
          from h' through the sqrt  |q| dh / (2 sqrt(h') D)
          sqrt, + delta, lr * gv and the divide round: 4 u |q|
      w'  one more rounding:        u (|w| + |q|)
    Both bounds are doubled to absorb the second-order terms."""
    n = 524291
    arena, s, (W, G, H) = _one_tensor(n, seed=700, h_abs=True)
    Wd, Gd, Hd = W.to(DEV), G.to(DEV), H.to(DEV)
    lr, delta, wd = 0.1, 1e-8, 1e-3
    ops.adagrad_update(*(arena.views(t)[0] for t in (Wd, Gd, Hd)),
                       lr, delta, wd)
    torch.cuda.synchronize()
    lr, delta, wd = _f32(lr), _f32(delta), _f32(wd)
    w, g, h = W[s].double(), G[s].double(), H[s].double()
    Wr, Hr = W.double().clone(), H.double().clone()
    Bw, Bh = torch.zeros_like(Wr), torch.zeros_like(Wr)
    gv = g + wd * w
    hn = h + gv * gv
    D = hn.sqrt() + delta
    q = lr * gv / D
    Hr[s], Wr[s] = hn, w - q
    dg = 2 * U * (g.abs() + (wd * w).abs())
    dh = 2 * gv.abs() * dg + U * gv * gv + U * (h + gv * gv)
    dq = lr * dg / D + q.abs() * dh / (2 * hn.sqrt() * D) + 4 * U * q.abs()
    Bh[s] = 2 * dh
    Bw[s] = 2 * (dq + U * (w.abs() + q.abs()))
    _check_within(Wd, Wr, Bw, "adagrad w")
    _check_within(Hd, Hr, Bh, "adagrad h")
    assert torch.equal(Gd.cpu(), G)


# ---------------------------------------------------------------------------
# D. repack_mt / unpack_mt with several tensors per table
# ---------------------------------------------------------------------------

# (x shape, w shape, pad, groups): a 3x3 conv whose 9216 weights cross a
# chunk and whose 288-wide rows are padded to 320; a grouped conv with its
# per-group dgrad transpose
_RP_CONVS = [((2, 32, 8, 8), (32, 32, 3, 3), 1, 1),
             ((2, 16, 8, 8), (16, 8, 3, 3), 1, 2)]
_RP_FC = (10, 1001)  # 10010 weights: the cast path, n % 4 = 2, two chunks


def _khwc_cols(Cig, kh, kw, kw_ld, c_ld):
    """Column of weight (ci, ky, kx) in a khwc row, in NCHW element order:
    (ky * kw_ld + kx) * c_ld + ci, as ps_khwc_col defines it."""
    ci = torch.arange(Cig).view(Cig, 1, 1)
    ky = torch.arange(kh).view(1, kh, 1)
    kx = torch.arange(kw).view(1, 1, kw)
    return ((ky * kw_ld + kx) * c_ld + ci).reshape(-1)


def test_repack_mt_several_tensors():
    masters, plans = [], []
    for k, (xs, ws, pad, G) in enumerate(_RP_CONVS):
        masters.append(torch.randn(*ws, generator=_gen(800 + k)))
        plans.append(ops.conv_plan(xs, ws, (1, 1), (pad, pad), G, True))
    assert plans[0]["wk_ld"] == 320 and plans[1]["wk_ld"] == 72
    N, K = _RP_FC
    masters.append(torch.randn(N, K, 1, 1, generator=_gen(810)))
    Gs = [c[3] for c in _RP_CONVS] + [1]
    kw_lds = [p["kw_ld"] for p in plans] + [1]
    c_lds = [p["c_ld"] for p in plans] + [K]
    for (xs, ws, _, G), kl, cl in zip(_RP_CONVS, kw_lds, c_lds):
        assert (kl, cl) == ops.khwc_layout(ws[1], ws[3], False)

    wk_shapes = [(m.shape[0], p["wk_ld"]) for m, p in zip(masters, plans)]
    wk_shapes.append((N, K))
    wkT_shapes = [(G * ws[2] * ws[3] * ws[1], ws[0] // G)
                  for _, ws, _, G in _RP_CONVS]
    a_wk = Arena([r * c for r, c in wk_shapes])
    a_wkT = Arena([r * c for r, c in wkT_shapes])
    # prior content: a bf16 ramp, so a pad column that was written shows
    wk0 = ((torch.arange(a_wk.total) % 251).float() - 125.0).to(torch.bfloat16)
    wkT0 = a_wkT.new(torch.bfloat16, fill=-3.0)

    # reference: a plain permutation of the bf16-rounded masters
    wk_ref, wkT_ref = wk0.clone(), wkT0.clone()
    for k, m in enumerate(masters):
        Co, Cig, kh, kw = m.shape
        rows = a_wk.views(wk_ref)[k].view(*wk_shapes[k])
        rows[:, _khwc_cols(Cig, kh, kw, kw_lds[k], c_lds[k])] = \
            m.reshape(Co, -1).to(torch.bfloat16)
    for k, (_, ws, _, G) in enumerate(_RP_CONVS):
        Co, Cig, kh, kw = ws
        a_wkT.views(wkT_ref)[k].copy_(
            masters[k].view(G, Co // G, Cig, kh, kw).permute(0, 3, 4, 2, 1)
            .reshape(-1).to(torch.bfloat16))

    md = [m.to(DEV) for m in masters]
    wkd, wkTd = wk0.to(DEV), wkT0.to(DEV)
    wks = [v.view(*s) for v, s in zip(a_wk.views(wkd), wk_shapes)]
    wkTs = [v.view(*s) for v, s in zip(a_wkT.views(wkTd), wkT_shapes)]
    wkTs.append(torch.empty(0, dtype=torch.bfloat16, device=DEV))
    mt = ops.repack_mt_prepare(md, wks, wkTs, Gs, kw_lds, c_lds)
    assert mt[2] == sum((m.numel() + MT_CHUNK - 1) // MT_CHUNK
                        for m in masters) == 5
    ops.repack_mt_run(mt)
    torch.cuda.synchronize()
    assert torch.equal(wkd.cpu(), wk_ref)
    assert torch.equal(wkTd.cpu(), wkT_ref)
    # said once more in the issue's words: the fc shadow is the cast master
    assert torch.equal(wks[2].cpu(),
                       masters[2].view(N, K).to(torch.bfloat16))
    for m, d in zip(masters, md):
        assert torch.equal(d.cpu(), m)


def test_unpack_mt_several_tensors():
    """dw += gather(dwk): one f32 add per element, so the result is exact.
    The pad columns of dwk hold garbage the gather must not read."""
    shapes = [c[1] for c in _RP_CONVS] + [(24, 16, 1, 1)]
    ldks = [ops.conv_plan(xs, ws, (1, 1), (pad, pad), G, True)["Kgw"]
            for xs, ws, pad, G in _RP_CONVS] + [16]
    layouts = [ops.khwc_layout(ws[1], ws[3], False) for ws in shapes]
    a_dwk = Arena([ws[0] * ld for ws, ld in zip(shapes, ldks)])
    a_dw = Arena([ws[0] * ws[1] * ws[2] * ws[3] for ws in shapes])
    dwk0 = torch.randn(a_dwk.total, generator=_gen(900))
    dw0 = a_dw.new()
    for k, s in enumerate(a_dw.slices()):
        dw0[s] = torch.randn(s.stop - s.start, generator=_gen(910 + k))
    dw_ref = dw0.clone()
    for k, (Co, Cig, kh, kw) in enumerate(shapes):
        rows = a_dwk.views(dwk0)[k].view(Co, ldks[k])
        gathered = rows[:, _khwc_cols(Cig, kh, kw, *layouts[k])]
        a_dw.views(dw_ref)[k].add_(gathered.reshape(-1))

    dwkd, dwd = dwk0.to(DEV), dw0.to(DEV)
    dwks = [v.view(ws[0], ld)
            for v, ws, ld in zip(a_dwk.views(dwkd), shapes, ldks)]
    dws = [v.view(*ws) for v, ws in zip(a_dw.views(dwd), shapes)]
    mt = ops.unpack_mt_prepare(dwks, dws, [ws[1] for ws in shapes],
                               [ws[2] for ws in shapes],
                               [ws[3] for ws in shapes],
                               [l[0] for l in layouts],
                               [l[1] for l in layouts])
    assert mt[2] == 2 + 1 + 1
    ops.unpack_mt_run(mt)
    torch.cuda.synchronize()
    assert torch.equal(dwd.cpu(), dw_ref)
    assert torch.equal(dwkd.cpu(), dwk0)


# ---------------------------------------------------------------------------
# E. colsum_acc and colsum_mt, exactly
# ---------------------------------------------------------------------------
# Inputs are multiples of 1/8 in [-4, 4] (exact in bf16 as well), db starts
# from such values too, so every partial sum in any order is a multiple of
# 1/8 below 2^21 in magnitude (4 R + |prefill| < 2^21 for every shape here)
# and f32 holds it exactly: the kernels must return the integer sums.

@functools.lru_cache(maxsize=2)
def _eighths(R, C):
    """x * 8 as int32 [R, C], asymmetric in row and column, and its column
    sums as int64."""
    x8 = torch.randint(-24, 25, (R, C), generator=_gen(R * 131 + C),
                       dtype=torch.int32)
    x8 += ((torch.arange(C, dtype=torch.int32) * 7) % 17 - 8).view(1, C)
    x8[R // 3] += 3  # one row unlike the others
    x8.clamp_(-32, 32)
    return x8, x8.sum(0, dtype=torch.int64)


def _prefill8(C):
    return ((torch.arange(C, dtype=torch.int64) * 5) % 23) - 11


def _colsum_route(R, C, vec):
    """The launcher's choice (ps_colsum_f32 / _bf16), recomputed."""
    from math import gcd
    if not (C % vec == 0 and C <= 8192
            and (R * C >= (8 << 20) or (R < 1024 and C >= 512))):
        return f"banded-{max(1, min(1024, R // 64))}blk"
    nvec = R * C // vec
    blocks = min(2048, (nvec + 255) // 256)
    rot = blocks * 256 * vec % C
    ph = C // gcd(rot, C) if rot else 1
    if ph > 4:
        return f"ph{ph}-banded"
    return f"flat-ph{ph}-{(nvec + blocks * 256 - 1) // (blocks * 256)}pass"


F32, BF16 = torch.float32, torch.bfloat16
_COLSUM_CASES = [
    (50, 130, F32, "banded-1blk"), (50, 130, BF16, "banded-1blk"),
    (200, 130, F32, "banded-3blk"), (200, 130, BF16, "banded-3blk"),
    (200, 67, F32, "banded-3blk"), (200, 67, BF16, "banded-3blk"),
    # C % 4 != 0: not eligible for the flat kernel
    (8, 514, F32, "banded-1blk"), (8, 514, BF16, "banded-1blk"),
    (8, 512, F32, "flat-ph1-1pass"), (8, 512, BF16, "flat-ph1-1pass"),
    (2, 768, F32, "flat-ph3-1pass"), (2, 768, BF16, "flat-ph3-1pass"),
    (1023, 4096, F32, "flat-ph1-2pass"), (1023, 4096, BF16, "flat-ph1-1pass"),
    (1023, 8192, F32, "flat-ph1-4pass"), (1023, 8192, BF16, "flat-ph1-2pass"),
    (1023, 3072, F32, "flat-ph3-2pass"),
    (1023, 6144, F32, "flat-ph3-3pass"), (1023, 6144, BF16, "flat-ph3-2pass"),
    # the big-matrix route at AlexNet conv1's C
    (87400, 96, F32, "flat-ph3-5pass"), (87400, 96, BF16, "flat-ph3-3pass"),
    (1023, 2560, F32, "ph5-banded"),
    (1023, 5120, F32, "ph5-banded"), (1023, 5120, BF16, "ph5-banded"),
]


@pytest.mark.parametrize(
    "R,C,dtype,route", _COLSUM_CASES,
    ids=[f"{R}x{C}-{'bf16' if d is BF16 else 'f32'}-{r}"
         for R, C, d, r in _COLSUM_CASES])
def test_colsum_acc_exact(R, C, dtype, route):
    assert _colsum_route(R, C, 8 if dtype is BF16 else 4) == route
    x8, sum8 = _eighths(R, C)
    assert 4 * R + 4 < 2 ** 21
    x = (x8.float() / 8).to(dtype).to(DEV)
    for pre8 in (_prefill8(C), torch.zeros(C, dtype=torch.int64)):
        arena = Arena([C])
        buf = arena.new()
        buf[arena.slices()[0]] = pre8.float() / 8
        want = buf.clone()
        want[arena.slices()[0]] = (pre8 + sum8).double().div(8).float()
        bufd = buf.to(DEV)
        ops.colsum_acc(x, arena.views(bufd)[0])
        torch.cuda.synchronize()
        assert torch.equal(bufd.cpu(), want), \
            f"{int((bufd.cpu() != want).sum())} of {C} columns differ"


# channels-last [N, C, H, W], largest C first, then smallest
_COLSUM_MT = {
    F32: [(2, 2048, 12, 12),   # nph == 0, three chunks, the last partial
          (2, 16, 100, 100),   # R = 20000 > rows_per = 16384; nph = 64
          (2, 24, 75, 75),     # CV = 6: 4 idle threads; two chunks
          (3, 1024, 10, 10)],  # nph = 1, rows_per = 256, two chunks
    BF16: [(2, 4096, 9, 9),    # nph == 0, three chunks
           (2, 24, 75, 75)],   # CV = 3: one idle thread; two chunks
}
_COLSUM_MT_CHUNKS = {F32: 3 + 2 + 2 + 2, BF16: 3 + 2}


@pytest.mark.parametrize("prefilled", [True, False], ids=["prefilled", "zero"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_colsum_mt_exact(dtype, prefilled):
    shapes = _COLSUM_MT[dtype]
    arena = Arena([s[1] for s in shapes])
    buf = arena.new()
    dys, sums, pres = [], [], []
    for (N, C, H, W), sl in zip(shapes, arena.slices()):
        x8, sum8 = _eighths(N * H * W, C)
        dy = (x8.float() / 8).to(dtype).to(DEV).view(N, H, W, C)
        dys.append(dy.permute(0, 3, 1, 2))
        pre8 = _prefill8(C) if prefilled else torch.zeros(C, dtype=torch.int64)
        buf[sl] = pre8.float() / 8
        sums.append(sum8)
        pres.append(pre8)
    bufd = buf.to(DEV)
    mt = ops.colsum_mt_prepare(dys, arena.views(bufd))
    assert mt[2] == _COLSUM_MT_CHUNKS[dtype] and mt[3] == shapes[0][1]
    for run in (1, 2):  # the second run accumulates onto the first
        ops.colsum_mt_run(mt, dtype is BF16)
        torch.cuda.synchronize()
        want = buf.clone()
        for sl, pre8, sum8 in zip(arena.slices(), pres, sums):
            want[sl] = (pre8 + run * sum8).double().div(8).float()
        assert torch.equal(bufd.cpu(), want), f"run {run}"


def test_colsum_mt_rejects_wide_and_mixed():
    def cl(N, C, H, W, dtype):
        return torch.zeros(N, H, W, C, dtype=dtype,
                           device=DEV).permute(0, 3, 1, 2)

    with pytest.raises(RuntimeError, match="LDS budget"):
        ops.colsum_mt_prepare([cl(1, 8200, 2, 2, F32)],
                              [torch.zeros(8200, device=DEV)])
    # one kernel instantiation reads every dy of a table
    with pytest.raises(RuntimeError, match="one dtype"):
        ops.colsum_mt_prepare(
            [cl(1, 16, 2, 2, F32), cl(1, 16, 2, 2, BF16)],
            [torch.zeros(16, device=DEV), torch.zeros(16, device=DEV)])
