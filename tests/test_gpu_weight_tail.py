"""The fused weight tail: fc weight gradients written straight into the param
diff, sole-owner diffs left out of the zero table, fc bf16 shadows written by
the SGD kernel, and the _version guard that falls back to the full repack.

Kernel tests compare whole sentinel-filled backing buffers, so a write outside
a tensor fails them too. Training tests run in deterministic mode, where the
steps repeat bit for bit, and ask for torch.equal."""

import pytest
import torch

import poseidon_amd as pa
from poseidon_amd.ops import functional as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 7777.0
NAN = float("nan")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


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

    def new(self, dtype=torch.float32, fill=SENTINEL):
        return torch.full((self.total,), fill, dtype=dtype)

    def views(self, buf):
        return [buf.narrow(0, s, n) for s, n in zip(self.starts, self.sizes)]


@pytest.fixture
def tail_switch():
    """Leaves the process-wide switch as it found it."""
    was = ops.fused_weight_tail()
    yield
    ops.set_fused_weight_tail(was)


# ---------------------------------------------------------------------------
# A. linear_backward writes dW into dw_out
# ---------------------------------------------------------------------------

def _linear_inputs(M, N, K, dtype, seed):
    x = torch.randn(M, K, generator=_gen(seed)).to(dtype)
    dy = torch.randn(M, N, generator=_gen(seed + 1)).to(dtype)
    w = torch.randn(N, K, generator=_gen(seed + 2))  # fp32 master
    return x.to(DEV), w.to(DEV), dy.to(DEV)


def _dw_into_nan(x, w, dy, N, K):
    """dW through dw_out, the target prefilled with NaN inside a sentinel
    arena; returns (target region, whole buffer, arena)."""
    arena = Arena([N * K])
    buf = arena.new().to(DEV)
    out = arena.views(buf)[0].view(N, K)
    out.fill_(NAN)
    dx, dw, db = ops.linear_backward(x, w, dy, False, True, False, dw_out=out)
    torch.cuda.synchronize()
    assert dx is None and dw is None and db is None
    guard = arena.new()
    arena.views(guard)[0].copy_(out.reshape(-1).cpu())
    assert torch.equal(buf.cpu(), guard), "write outside dw_out"
    return out


@pytest.mark.parametrize("name", ["fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", [(8, 72, 200), (5, 1000, 136)])
def test_dw_out_equals_returned_dw(M, N, K, name):
    """Shapes ragged against every tile. beta 0 into the NaN-filled target
    must give the bits the allocating call returns."""
    x, w, dy = _linear_inputs(M, N, K, DTYPES[name], 100 + M)
    _, dw_ref, _ = ops.linear_backward(x, w, dy, False, True, False)
    out = _dw_into_nan(x, w, dy, N, K)
    assert torch.equal(out, dw_ref)


@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_dw_out_splitk_target_not_assumed_zero(name):
    """A split-K dW plan (atomic accumulation into the target) with the
    target prefilled with NaN: the plan must clear it itself. Reference: fp64
    from the values the kernel reads; bounds: those of test_gemm_layouts
    (fp32, contraction >= 4096: 1e-3) and test_gemm_bf16_layouts (rtol 1e-2,
    atol 3e-2)."""
    N = K = 64
    bf16 = name == "bf16"
    M = next((m for m in (4608, 9216, 18432)
              if ops.gemm_plan(N, K, m, False, False, bf16)["splitk"] > 1),
             None)
    assert M is not None, "no split-K plan from batch 4608 upwards"
    x, w, dy = _linear_inputs(M, N, K, DTYPES[name], 300)
    ref = dy.double().t().cpu() @ x.double().cpu()
    out = _dw_into_nan(x, w, dy, N, K).cpu().double()
    assert bool(torch.isfinite(out).all()), "NaN prefill leaked into dW"
    err = (out - ref).abs()
    rel = (err / ref.abs().clamp(min=1.0)).max().item()
    rtol, atol = (1e-2, 3e-2) if bf16 else (1e-3, 1e-3)
    print(f"{name} M={M}: max abs {err.max().item():.3e} rel {rel:.3e}")
    assert rel <= rtol or err.max().item() <= atol


# ---------------------------------------------------------------------------
# B. sgd_mt writes bf16 shadows
# ---------------------------------------------------------------------------

_SGD_SIZES = [1, 3, 4, 5, 8191, 8192, 8193, 2 * 8192 + 5]


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("lr_on_device", [False, True])
def test_sgd_mt_shadows(parity, lr_on_device):
    """Every second tensor (either parity) gets a shadow. w and h must match
    a run without shadows bit for bit, each shadow must be w.to(bf16), and
    the slots of the tensors without a shadow, like the guard elements
    around every slot, must keep their sentinels."""
    arena = Arena(_SGD_SIZES)
    W0 = arena.new()
    G0 = arena.new()
    H0 = arena.new()
    for k, (w, g, h) in enumerate(zip(arena.views(W0), arena.views(G0),
                                      arena.views(H0))):
        w.copy_(torch.randn(w.numel(), generator=_gen(10 + k)))
        g.copy_(torch.randn(w.numel(), generator=_gen(30 + k)) * 0.1)
        h.copy_(torch.randn(w.numel(), generator=_gen(50 + k)) * 0.01)
    nt = len(_SGD_SIZES)
    lr_mults = [1.0 + 0.5 * (k % 3) for k in range(nt)]
    wds = [0.0005 * (k % 2) for k in range(nt)]
    lr, mom = 0.05, 0.9
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=DEV) \
        if lr_on_device else None

    def run(with_shadows):
        Wd, Gd, Hd = W0.to(DEV), G0.to(DEV), H0.to(DEV)
        Sd = arena.new(torch.bfloat16).to(DEV)
        shadows = None
        if with_shadows:
            shadows = [s if k % 2 == parity else None
                       for k, s in enumerate(arena.views(Sd))]
        mt = ops.sgd_mt_prepare(arena.views(Wd), arena.views(Gd),
                                arena.views(Hd), lr_mults, wds, shadows)
        ops.sgd_mt_run(mt, 0.0 if lr_on_device else lr, mom, lr_dev)
        torch.cuda.synchronize()
        return Wd.cpu(), Gd.cpu(), Hd.cpu(), Sd.cpu()

    W1, G1, H1, S1 = run(False)
    W2, G2, H2, S2 = run(True)
    assert not torch.equal(W1, W0)  # the update did something
    assert torch.equal(W2, W1) and torch.equal(H2, H1)
    assert torch.equal(G2, G0) and torch.equal(G1, G0)
    assert torch.equal(S1, arena.new(torch.bfloat16))
    S_ref = arena.new(torch.bfloat16)
    for k, (s, w) in enumerate(zip(arena.views(S_ref), arena.views(W1))):
        if k % 2 == parity:
            s.copy_(w.to(torch.bfloat16))
    assert torch.equal(S2, S_ref)


# ---------------------------------------------------------------------------
# C. unpack_mt overwrite
# ---------------------------------------------------------------------------

def _khwc_cols(Cig, kh, kw, kw_ld, c_ld):
    """Column of weight (ci, ky, kx) in a khwc row, in NCHW element order."""
    ci = torch.arange(Cig).view(Cig, 1, 1)
    ky = torch.arange(kh).view(1, kh, 1)
    kx = torch.arange(kw).view(1, 1, kw)
    return ((ky * kw_ld + kx) * c_ld + ci).reshape(-1)


def test_unpack_mt_overwrite_and_default():
    """Two convs, one with 3x3 taps and an ldk padded past its 288 columns.
    Overwrite: dw, prefilled with NaN, becomes the permuted dwk exactly. The
    default still adds to what dw holds."""
    shapes = [(32, 32, 3, 3), (24, 16, 1, 1)]
    ldks = [ops.conv_plan((2, 32, 8, 8), shapes[0], (1, 1), (1, 1), 1,
                          True)["Kgw"], 16]
    assert ldks[0] > 32 * 9
    layouts = [ops.khwc_layout(ws[1], ws[3], False) for ws in shapes]
    a_dwk = Arena([ws[0] * ld for ws, ld in zip(shapes, ldks)])
    a_dw = Arena([ws[0] * ws[1] * ws[2] * ws[3] for ws in shapes])
    dwk0 = torch.randn(a_dwk.total, generator=_gen(900))
    gathered = []
    for k, (Co, Cig, kh, kw) in enumerate(shapes):
        rows = a_dwk.views(dwk0)[k].view(Co, ldks[k])
        gathered.append(rows[:, _khwc_cols(Cig, kh, kw, *layouts[k])]
                        .reshape(-1))
    prefill = [torch.randn(g.numel(), generator=_gen(910 + k))
               for k, g in enumerate(gathered)]

    def run(overwrite):
        dw0 = a_dw.new()
        for v, p in zip(a_dw.views(dw0), prefill):
            v.copy_(torch.full_like(p, NAN) if overwrite else p)
        dwkd, dwd = dwk0.to(DEV), dw0.to(DEV)
        dwks = [v.view(ws[0], ld)
                for v, ws, ld in zip(a_dwk.views(dwkd), shapes, ldks)]
        dws = [v.view(*ws) for v, ws in zip(a_dw.views(dwd), shapes)]
        args = ([ws[1] for ws in shapes], [ws[2] for ws in shapes],
                [ws[3] for ws in shapes], [l[0] for l in layouts],
                [l[1] for l in layouts])
        mt = ops.unpack_mt_prepare(dwks, dws, *args, [True, True]) \
            if overwrite else ops.unpack_mt_prepare(dwks, dws, *args)
        ops.unpack_mt_run(mt)
        torch.cuda.synchronize()
        assert torch.equal(dwkd.cpu(), dwk0)
        return dwd.cpu()

    ref = a_dw.new()
    for v, g in zip(a_dw.views(ref), gathered):
        v.copy_(g)
    assert torch.equal(run(True), ref)
    for v, g, p in zip(a_dw.views(ref), gathered, prefill):
        v.copy_(p + g)
    assert torch.equal(run(False), ref)


# ---------------------------------------------------------------------------
# D. training with the switch on equals training with it off
# ---------------------------------------------------------------------------

_HEAD = """
    name: "tailnet"
    layers { name: "data" type: DUMMY_DATA top: "data" top: "label"
             dummy_data_param { num: 8 channels: 3 height: 12 width: 12
                 num: 8 channels: 1 height: 1 width: 1
                 data_filler { type: "gaussian" std: 1.0 }
                 data_filler { type: "constant" } } }
    layers { name: "c1" type: CONVOLUTION bottom: "data" top: "c1"
             blobs_lr: 1 blobs_lr: 2 weight_decay: 1 weight_decay: 0
             convolution_param { num_output: 4 kernel_size: 3
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "ip1" type: INNER_PRODUCT bottom: "c1" top: "ip1"
             inner_product_param { num_output: 16
                 weight_filler { type: "gaussian" std: 0.05 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "r1" type: RELU bottom: "ip1" top: "ip1" }
"""
_PLAIN = _HEAD + """
    layers { name: "ip2" type: INNER_PRODUCT bottom: "ip1" top: "ip2"
             inner_product_param { num_output: 10
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" } } }
    layers { name: "loss" type: SOFTMAX_LOSS bottom: "ip2" bottom: "label"
             top: "loss" }
"""
# ip3 shares ip2's weight (not its bias): two writers per backward
_SHARED = _HEAD + """
    layers { name: "ip2" type: INNER_PRODUCT bottom: "ip1" top: "ip2"
             param: "w2"
             inner_product_param { num_output: 10
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" } } }
    layers { name: "ip3" type: INNER_PRODUCT bottom: "ip1" top: "ip3"
             param: "w2"
             inner_product_param { num_output: 10
                 weight_filler { type: "gaussian" std: 0.1 }
                 bias_filler { type: "constant" value: 0.2 } } }
    layers { name: "loss" type: SOFTMAX_LOSS bottom: "ip2" bottom: "label"
             top: "loss" }
    layers { name: "loss3" type: SOFTMAX_LOSS bottom: "ip3" bottom: "label"
             top: "loss3" }
"""


def _feed(net, dtype):
    data = torch.randn(8, 3, 12, 12, generator=_gen(17)) \
        .to(torch.bfloat16).float()
    labels = torch.tensor([0.0, 2.0, 4.0, 1.0, 9.0, 7.0, 3.0, 3.0])
    net.blobs["data"].data = data.to(DEV, dtype)
    net.blobs["label"].data = labels.view(8, 1, 1, 1).to(DEV)
    net.layers[0]._filled = True
    net.layers[0].refill = [False, False]


def _solver(text, graphed, prefix=""):
    from poseidon_amd.proto import Message, parse_text
    from poseidon_amd.solver.solver import SGDSolver
    sp = Message("SolverParameter", base_lr=0.05, lr_policy="fixed",
                 momentum=0.9, weight_decay=0.001, max_iter=100, display=0,
                 snapshot=0)
    if prefix:
        sp.snapshot_prefix = prefix
    sp.net_param = parse_text("NetParameter", text)
    s = SGDSolver(sp, verbose=False)
    _feed(s.net, pa.ctx().compute_dtype)
    if graphed:
        assert s.enable_graph() is True
    return s


def _owned(s):
    return [i for i, ps in enumerate(s.net.params) if ps.owner == i]


def _state(s, graphed):
    torch.cuda.synchronize()
    if graphed:  # a capture that failed falls back to eager and clears these
        assert s._use_graph and s._graph is not None
    return {kind: [t.detach().cpu().clone() for t in ts] for kind, ts in (
        ("weight", [s.net.params[i].blob.data for i in _owned(s)]),
        ("history", [s.history[i] for i in _owned(s)]),
        ("diff", [s.net.params[i].blob.diff for i in _owned(s)]))}


def _assert_same_state(a, b, what):
    for kind in a:
        for k, (x, y) in enumerate(zip(a[kind], b[kind])):
            assert torch.equal(x, y), \
                f"{what}: {kind} {k} differs, max " \
                f"{(x.double() - y.double()).abs().max().item():.3e}"


class _Det:
    """Deterministic GPU context for one test, then back to the CPU one."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        pa.init(device="cuda", seed=1234, compute_dtype=self.dtype,
                deterministic=True)

    def __exit__(self, *exc):
        pa.init(device="cpu", compute_dtype=torch.float32,
                deterministic=False)


def _train5(text, dtype, graphed, switch):
    ops.set_fused_weight_tail(switch)
    with _Det(dtype):
        s = _solver(text, graphed)
        s.step(5)
        st = _state(s, graphed)
        net = s.net
        lay = {l.name: l for l in net.layers}
        zeroed = set(net._zero_mt[1])
        info = {
            "over": {n: l.overwrites_dw() for n, l in lay.items()
                     if hasattr(l, "overwrites_dw")},
            "zeroed": {n: id(l.blobs[0].diff) in zeroed
                       for n, l in lay.items() if l.blobs},
            "bias_zeroed": all(id(l.blobs[1].diff) in zeroed
                               for l in lay.values() if len(l.blobs) > 1),
            "shadows_current": net.fc_shadows_current(),
            "shadow_layers": [l.name for l in s._shadow_layers],
        }
        return st, info


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_training_same_with_switch_on_and_off(name, graphed, shared,
                                              tail_switch):
    """Five SGD steps (momentum, weight decay) leave every weight, history
    and diff equal whether the tail is fused or not -- and the fused run
    really took the other path: sole-owner weight diffs are out of the zero
    table, a shared weight stays in it and keeps accumulating."""
    text = _SHARED if shared else _PLAIN
    off, i_off = _train5(text, DTYPES[name], graphed, False)
    on, i_on = _train5(text, DTYPES[name], graphed, True)
    _assert_same_state(on, off, f"{name} graphed={graphed} shared={shared}")

    assert not any(i_off["over"].values())
    assert all(i_off["zeroed"].values()) and not i_off["shadows_current"]
    assert i_off["shadow_layers"] == []
    sole = ["c1", "ip1"] + ([] if shared else ["ip2"])
    for n in sole:
        assert i_on["over"][n] and not i_on["zeroed"][n], n
    if shared:
        for n in ("ip2", "ip3"):
            assert not i_on["over"][n], n
        assert i_on["zeroed"]["ip2"], "shared weight left the zero table"
    assert i_on["bias_zeroed"] and i_off["bias_zeroed"]
    if name == "bf16":
        # the owner's shadow rides the update; a sharer keeps the repack
        assert i_on["shadow_layers"] == ["ip1", "ip2"]
        assert i_on["shadows_current"]
    else:
        assert i_on["shadow_layers"] == []


def test_bare_backward_twice_accumulates(tail_switch):
    """Without a solver nothing is marked: a second forward / backward
    without zeroing doubles the fc weight and bias diffs, switch on."""
    from poseidon_amd.core.net import Net, TRAIN
    from poseidon_amd.proto import parse_text
    ops.set_fused_weight_tail(True)
    with _Det(torch.bfloat16):
        net = Net(parse_text("NetParameter", _PLAIN), phase=TRAIN,
                  verbose=False)
        _feed(net, torch.bfloat16)
        net.forward()
        net.zero_param_diffs()
        net.backward()
        ips = [l for l in net.layers if l.type_name == "INNER_PRODUCT"]
        assert len(ips) == 2 and not any(l.overwrites_dw() for l in ips)
        once = [b.diff.clone() for l in ips for b in l.blobs]
        net.forward()  # a backward consumes what its forward kept
        net.backward()
        twice = [b.diff for l in ips for b in l.blobs]
        for a, b in zip(once, twice):
            assert bool(a.abs().max() > 0) and torch.equal(b, a * 2)


# ---------------------------------------------------------------------------
# E. the _version guard: masters written behind the solver's back
# ---------------------------------------------------------------------------

def _first_step_from(w0, graphed):
    """A fresh solver's first step from the weights w0."""
    s = _solver(_PLAIN, graphed)
    for i, w in zip(_owned(s), w0):
        s.net.params[i].blob.data.copy_(w)
    s.step(1)
    return _state(s, graphed)["weight"]


@pytest.mark.parametrize("graphed,how", [
    (False, "rewind"), (True, "rewind"),
    (False, "load_weights"), (True, "load_weights"),
    # eager only: restore() rebinds the history tensors, which a captured
    # graph cannot follow, with or without the fused tail
    (False, "restore")])
def test_stale_shadows_are_refreshed(graphed, how, tail_switch, tmp_path):
    """Three steps, then the weights go back to the start behind the
    solver's back and the histories to zero; the next step must read
    shadows of the weights that are there now, not the ones the last update
    wrote. rewind: copy_ / zero_ in place, as a benchmark harness does.
    load_weights / restore: from a snapshot taken at iteration 0 (both copy
    into the master tensors in place, which bumps their _version)."""
    ops.set_fused_weight_tail(True)
    with _Det(torch.bfloat16):
        s = _solver(_PLAIN, graphed, prefix=str(tmp_path / "snap"))
        w0 = [s.net.params[i].blob.data.clone() for i in _owned(s)]
        model = s.snapshot() if how != "rewind" else None
        s.step(3)
        assert s.net.fc_shadows_current()
        if how == "rewind":
            for i, w in zip(_owned(s), w0):
                s.net.params[i].blob.data.copy_(w)
            for h in s.history.values():
                h.zero_()
        elif how == "load_weights":
            s.load_weights(model)
            for h in s.history.values():
                h.zero_()
        else:
            s.restore(model.replace(".caffemodel", ".solverstate"))
            assert s.iter == 0
        assert not s.net.fc_shadows_current()
        s.step(1)
        got = _state(s, graphed)["weight"]
        assert s.net.fc_shadows_current()
        ref = _first_step_from(w0, graphed)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), \
            f"weight {k}: max {(a.double() - b.double()).abs().max():.3e}"
