"""Dense softmax microbench: the lane-group kernels (softmax_dense.hip,
softmax_heads.hip) against the wave-per-row kernels run with rows = N*H*W, in
one process -- the per-position loss, the plain 4-D softmax, each forward and
backward, and the per-position accuracy. Usage:

    python -m poseidon_amd.tools.softmax_bench
        [--shapes 32,21,256,256:32,2,512,512] [--dtype bf16] [--reps 20]
        [--rounds 2] [--top-k 3]

Per shape it checks both paths against a float64 evaluation of the
definition first (on the GPU: the blobs are too large to be worth a trip to
the host), then alternates switch off / on for --rounds rounds; every round
ramps the clocks for 100 ms and times --reps forward + backward pairs with
device events. A time is a call on the stream, output allocations included.
Printed: the median of each direction and, for both paths, the rate over the
bytes the operation must move -- logits in and prob out forward, prob in and
dx out backward, the fp32 labels each way; x in and y out, then y and dy in
and dx out for the plain softmax -- with the on path's share of --stream-gbs,
the HBM streaming rate. The accuracy kernel has no wave-per-row partner below
softmax_dense_max_c() worth the name; it is timed in the same loop as the
torch composite it replaces (topk over the row view, compare, mean), after
its count is checked against a float64 rank count.
"""

import argparse
import statistics
import time

import torch
import torch.nn.functional as F


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32,21,256,256:32,2,512,512")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--top-k", type=int, default=3)
    ap.add_argument("--stream-gbs", type=float, default=6300.0)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "softmax_bench needs a GPU"
    from poseidon_amd.ops import functional as ops
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    g = torch.Generator(device="cuda").manual_seed(0)

    def measure(first, second):
        """times of first() and of second(what first returned), in pairs"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.1:  # clock ramp
            second(first())
            torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)]
              for _ in range(args.reps)]
        for e in ev:
            e[0].record()
            out = first()
            e[1].record()
            second(out)
            e[2].record()
        torch.cuda.synchronize()
        return ([e[0].elapsed_time(e[1]) for e in ev],
                [e[1].elapsed_time(e[2]) for e in ev])

    def ab(first, second):
        """medians (off first, off second, on first, on second)"""
        t = {False: ([], []), True: ([], [])}
        for _ in range(args.rounds):
            for on in (False, True):
                ops.set_softmax_dense(on)
                a, b = measure(first, second)
                t[on][0].extend(a)
                t[on][1].extend(b)
        return [statistics.median(v) for v in
                (t[False][0], t[False][1], t[True][0], t[True][1])]

    def report(what, spec, fbytes, bbytes, times, tail):
        of, ob, nf, nb = times
        print(f"{what} {spec.replace(',', 'x')} {args.dtype} "
              f"({fbytes / 1e6:.1f} / {bbytes / 1e6:.1f} MB fwd / bwd): off "
              f"{of * 1e3:.1f} + {ob * 1e3:.1f} us = {fbytes / of / 1e6:.0f} "
              f"/ {bbytes / ob / 1e6:.0f} GB/s fwd / bwd, on {nf * 1e3:.1f} "
              f"+ {nb * 1e3:.1f} us = {fbytes / nf / 1e6:.0f} / "
              f"{bbytes / nb / 1e6:.0f} GB/s "
              f"({fbytes / nf / 1e6 / args.stream_gbs:.2f} / "
              f"{bbytes / nb / 1e6 / args.stream_gbs:.2f} of "
              f"{args.stream_gbs:.0f}), ratio fwd {of / nf:.2f}x bwd "
              f"{ob / nb:.2f}x; {tail}")

    was = ops.softmax_dense()
    for spec in args.shapes.split(":"):
        n, c, h, w = (int(v) for v in spec.split(","))
        rows = n * h * w
        x = (torch.randn(n, c, h, w, device="cuda", generator=g) * 4).to(dt) \
            .contiguous(memory_format=torch.channels_last)
        labels = torch.randint(0, c, (rows,), device="cuda",
                               generator=g).float()
        idx = labels.view(n, 1, h, w).long()
        nbytes = x.numel() * x.element_size()
        try:
            # -- the per-position loss ------------------------------------
            logp = F.log_softmax(x.double(), dim=1)
            ref_loss = -logp.gather(1, idx).mean().item()
            ref_dx = (logp.exp() - torch.zeros_like(logp)
                      .scatter_(1, idx, 1.0)) / rows
            del logp
            err = {}
            for on in (True, False):
                ops.set_softmax_dense(on)
                n0 = ops.softmax_dense_launches()
                loss, prob = ops.softmax_loss_forward(x, labels)
                dx = ops.softmax_loss_backward(prob, labels, 1.0)
                launches = ops.softmax_dense_launches() - n0
                assert launches == (2 if on else 0), \
                    f"C = {c} is outside the lane-group kernels"
                err[on] = (abs(loss.item() - ref_loss),
                           (dx.double() - ref_dx).abs().max().item() * rows)
                del prob, dx
            del ref_dx
            times = ab(lambda: ops.softmax_loss_forward(x, labels)[1],
                       lambda p: ops.softmax_loss_backward(p, labels, 1.0))
            report("loss", spec, 2 * nbytes + 4 * rows, 2 * nbytes + 4 * rows,
                   times, f"loss err on {err[True][0]:.3g} off "
                   f"{err[False][0]:.3g}, max |dx| err x rows on "
                   f"{err[True][1]:.3g} off {err[False][1]:.3g}")

            # -- the plain softmax ----------------------------------------
            dy = torch.randn(n, c, h, w, device="cuda", generator=g).to(dt) \
                .contiguous(memory_format=torch.channels_last)
            ref_y = F.softmax(x.double(), dim=1)
            for on in (True, False):
                ops.set_softmax_dense(on)
                n0 = ops.softmax_dense_launches()
                y = ops.softmax_forward(x)
                dx = ops.softmax_backward(y, dy)
                assert ops.softmax_dense_launches() - n0 == (2 if on else 0)
                yd = y.double()
                ref_dx = (dy - (dy * yd).sum(dim=1, keepdim=True)) * yd
                err[on] = ((yd - ref_y).abs().max().item(),
                           (dx.double() - ref_dx).abs().max().item())
                del y, dx, yd, ref_dx
            del ref_y
            times = ab(lambda: ops.softmax_forward(x),
                       lambda y: ops.softmax_backward(y, dy))
            report("softmax", spec, 2 * nbytes, 3 * nbytes, times,
                   f"max |y| err on {err[True][0]:.3g} off {err[False][0]:.3g}"
                   f", max |dx| err on {err[True][1]:.3g} off "
                   f"{err[False][1]:.3g}")
            del dy

            # -- the per-position accuracy --------------------------------
            k = min(args.top_k, c)
            xr = x.permute(0, 2, 3, 1).reshape(rows, c)
            lbl = labels.long().view(-1, 1)
            v = xr.gather(1, lbl)
            ahead = (xr > v) | ((xr == v) & (torch.arange(
                c, device="cuda").view(1, -1) > lbl))
            want = int((ahead.sum(dim=1) < k).sum().item())
            del ahead, v
            ops.set_softmax_dense(True)
            got = round(ops.accuracy(x, labels, k).item() * rows)
            assert got == want, f"accuracy counts {got}, rank count {want}"

            def composite(_):
                hit = (xr.topk(k, dim=1).indices == lbl).any(dim=1)
                return hit.float().sum() / rows

            ta, tc = (statistics.median(t) for t in measure(
                lambda: ops.accuracy(x, labels, k), composite))
            abytes = nbytes + 4 * rows
            print(f"accuracy {spec.replace(',', 'x')} {args.dtype} top_k {k} "
                  f"({abytes / 1e6:.1f} MB): kernel {ta * 1e3:.1f} us = "
                  f"{abytes / ta / 1e6:.0f} GB/s "
                  f"({abytes / ta / 1e6 / args.stream_gbs:.2f} of "
                  f"{args.stream_gbs:.0f}), torch topk composite "
                  f"{tc * 1e3:.1f} us; {got} of {rows} right")
            del xr
        finally:
            ops.set_softmax_dense(was)


if __name__ == "__main__":
    main()
