"""Dense softmax-loss microbench: the lane-group kernels (softmax_dense.hip)
against the wave-per-row kernels run with rows = N*H*W, forward and backward,
in one process. Usage:

    python -m poseidon_amd.tools.softmax_bench
        [--shapes 32,21,256,256:32,2,512,512] [--dtype bf16] [--reps 20]
        [--rounds 2]

Per shape it checks both paths against a float64 evaluation of the
definition first (on the GPU: the blobs are too large to be worth a trip to
the host), then alternates switch off / on for --rounds rounds; every round
ramps the clocks for 100 ms and times --reps forward + backward pairs with
device events. A time is a call on the stream, output allocations included.
Printed: the median of each direction and, for both paths, the rate over the
bytes the operation must move -- logits in and prob out forward, prob in and
dx out backward, the fp32 labels each way -- with the on path's share of
--stream-gbs, the HBM streaming rate.
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
    ap.add_argument("--stream-gbs", type=float, default=6300.0)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "softmax_bench needs a GPU"
    from poseidon_amd.ops import functional as ops
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    g = torch.Generator(device="cuda").manual_seed(0)

    def measure(x, labels):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.1:  # clock ramp
            _, prob = ops.softmax_loss_forward(x, labels)
            ops.softmax_loss_backward(prob, labels, 1.0)
            torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)]
              for _ in range(args.reps)]
        for e in ev:
            e[0].record()
            _, prob = ops.softmax_loss_forward(x, labels)
            e[1].record()
            ops.softmax_loss_backward(prob, labels, 1.0)
            e[2].record()
        torch.cuda.synchronize()
        return ([e[0].elapsed_time(e[1]) for e in ev],
                [e[1].elapsed_time(e[2]) for e in ev])

    was = ops.softmax_dense()
    for spec in args.shapes.split(":"):
        n, c, h, w = (int(v) for v in spec.split(","))
        rows = n * h * w
        x = (torch.randn(n, c, h, w, device="cuda", generator=g) * 4).to(dt) \
            .contiguous(memory_format=torch.channels_last)
        labels = torch.randint(0, c, (rows,), device="cuda",
                               generator=g).float()
        idx = labels.view(n, 1, h, w).long()
        logp = F.log_softmax(x.double(), dim=1)
        ref_loss = -logp.gather(1, idx).mean().item()
        ref_dx = (logp.exp() - torch.zeros_like(logp).scatter_(1, idx, 1.0)) \
            / rows
        del logp
        try:
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
            t = {False: ([], []), True: ([], [])}
            for _ in range(args.rounds):
                for on in (False, True):
                    ops.set_softmax_dense(on)
                    f, b = measure(x, labels)
                    t[on][0].extend(f)
                    t[on][1].extend(b)
        finally:
            ops.set_softmax_dense(was)
        nbytes = 2 * x.numel() * x.element_size() + 4 * rows  # each direction
        of, ob, nf, nb = (statistics.median(v) for v in
                          (t[False][0], t[False][1], t[True][0], t[True][1]))
        gbs = lambda ms: nbytes / ms / 1e6  # noqa: E731
        print(f"{spec.replace(',', 'x')} {args.dtype} ({nbytes / 1e6:.1f} MB "
              f"each way): off {of * 1e3:.1f} + {ob * 1e3:.1f} us = "
              f"{gbs(of):.0f} / {gbs(ob):.0f} GB/s fwd / bwd, on "
              f"{nf * 1e3:.1f} + {nb * 1e3:.1f} us = {gbs(nf):.0f} / "
              f"{gbs(nb):.0f} GB/s ({gbs(nf) / args.stream_gbs:.2f} / "
              f"{gbs(nb) / args.stream_gbs:.2f} of {args.stream_gbs:.0f}), "
              f"ratio {(of + ob) / (nf + nb):.2f}x; loss err on "
              f"{err[True][0]:.3g} off {err[False][0]:.3g}, max |dx| err x "
              f"rows on {err[True][1]:.3g} off {err[False][1]:.3g}")


if __name__ == "__main__":
    main()
