"""MVN microbench: the fused kernels (mvn.hip) against the tensor-op
composite, forward and backward, in one process. Usage:

    python -m poseidon_amd.tools.mvn_bench [--shapes 32,64,56,56:256,4096]
        [--dtype bf16] [--reps 20] [--rounds 2]

Per shape and mode (per channel, across channels) it checks the fused result
against an fp64 reference on the CPU first, then alternates switch off / on
for --rounds rounds; every round ramps the clocks for 100 ms and times
--reps forward + backward pairs with device events. Printed: the median of
each direction, the pair's ratio, and the fused kernels' rate over the bytes
the operation must move (x in and y out forward; x, dy in and dx out
backward) -- a split plan's second read is not counted, so its rate reads
low by design. A 2-D shape (N, K) runs as (N, K, 1, 1), which the composite
needs and which is the same memory.
"""

import argparse
import statistics
import time

import torch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32,64,56,56:256,4096")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "mvn_bench needs a GPU"
    from poseidon_amd.ops import functional as ops
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(0)

    def pair(x, dy, across):
        y, saved = ops.mvn_forward(x, across, True)
        return y, ops.mvn_backward(x, dy, saved, across, True, y=y)

    def measure(x, dy, across):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.1:  # clock ramp
            pair(x, dy, across)
            torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)]
              for _ in range(args.reps)]
        for e in ev:
            e[0].record()
            y, saved = ops.mvn_forward(x, across, True)
            e[1].record()
            ops.mvn_backward(x, dy, saved, across, True, y=y)
            e[2].record()
        torch.cuda.synchronize()
        return ([e[0].elapsed_time(e[1]) for e in ev],
                [e[1].elapsed_time(e[2]) for e in ev])

    for spec in args.shapes.split(":"):
        shape = tuple(int(v) for v in spec.split(","))
        shape4 = shape + (1,) * (4 - len(shape))
        xc = (1.0 + 0.5 * torch.randn(*shape4, generator=g)).to(dt)
        dc = torch.randn(*shape4, generator=g).to(dt)
        x = xc.to("cuda").contiguous(memory_format=torch.channels_last)
        dy = dc.to("cuda").contiguous(memory_format=torch.channels_last)
        nbytes = xc.numel() * xc.element_size()
        for across in (False, True):
            dims = (1, 2, 3) if across else (2, 3)
            xd, dd = xc.double(), dc.double()
            mean = xd.mean(dims, keepdim=True)
            rstd = 1 / (((xd - mean) ** 2).mean(dims, keepdim=True)
                        + 1e-10).sqrt()
            ry = (xd - mean) * rstd
            rdx = (dd - dd.mean(dims, keepdim=True)
                   - ry * (dd * ry).mean(dims, keepdim=True)) * rstd
            ops.set_mvn_fused(True)
            try:
                n0 = ops.mvn_launches()
                y, dx = pair(x, dy, across)
                launches = ops.mvn_launches() - n0
                ey = (y.cpu().double() - ry).abs().max().item()
                ex = (dx.cpu().double() - rdx).abs().max().item()
                t = {False: ([], []), True: ([], [])}
                for _ in range(args.rounds):
                    for on in (False, True):
                        ops.set_mvn_fused(on)
                        f, b = measure(x, dy, across)
                        t[on][0].extend(f)
                        t[on][1].extend(b)
            finally:
                ops.set_mvn_fused(True)
            cf, cb, ff, fb = (statistics.median(v) for v in
                              (t[False][0], t[False][1], t[True][0],
                               t[True][1]))
            print(f"{'x'.join(map(str, shape))} {args.dtype} "
                  f"{'across' if across else 'per-channel'}: composite "
                  f"{cf * 1e3:.1f} + {cb * 1e3:.1f} us, fused {ff * 1e3:.1f} "
                  f"+ {fb * 1e3:.1f} us ({launches} launches), ratio "
                  f"{(cf + cb) / (ff + fb):.2f}x, fused "
                  f"{2 * nbytes / ff / 1e6:.0f} / {3 * nbytes / fb / 1e6:.0f} "
                  f"GB/s fwd / bwd, max err y {ey:.3g} dx {ex:.3g}")


if __name__ == "__main__":
    main()
