"""GEMM kernel microbench (within-probe repeats, random data -- guide §5.4
rules 24/25). Usage:

    python -m poseidon_amd.tools.gemm_bench [--size 4096] [--dtype bf16]
        [--layout nt|nn|tn] [--reps 20] [--split] [--nn-ab]

--split (fp32 only) times the exact fp32 path and then the split-precision
path (ops.set_fp32_split) in the same process after one clock ramp, and
prints both with their ratio; TF/s is effective, from the fp32 FLOP count.

Every run prints the path its plan takes (generic, tr16, tr16_nn, split3).
--layout nn picks up the NN tr16 switch from PS_TR16_NN; --nn-ab (bf16, nn)
times the switch off and then on in the same process after one clock ramp
each. The test entry's C is f32: for the bf16-out plans of linear_backward's
dx, time ops.linear_backward itself.
"""

import argparse
import time

import torch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--mnk", default="", help="M,N,K override")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--layout", default="nt", choices=["nt", "nn", "tn"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--split", action="store_true",
                    help="also time the bf16x3 split path (needs --dtype fp32)")
    ap.add_argument("--nn-ab", action="store_true",
                    help="time the NN tr16 switch off, then on (bf16, nn)")
    args = ap.parse_args(argv)
    if args.split and args.dtype != "fp32":
        ap.error("--split is valid with --dtype fp32 only")
    if args.nn_ab and (args.dtype, args.layout) != ("bf16", "nn"):
        ap.error("--nn-ab is valid with --dtype bf16 --layout nn only")

    from poseidon_amd.ops._backend import load
    ext = load()
    if args.mnk:
        M, N, K = (int(x) for x in args.mnk.split(","))
    else:
        M = N = K = args.size
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    ak, bk = {"nt": (True, True), "nn": (True, False),
              "tn": (False, False)}[args.layout]

    g = torch.Generator().manual_seed(0)
    opA = torch.randn(M, K, generator=g)
    opB = torch.randn(K, N, generator=g)
    A = (opA if ak else opA.t()).contiguous().to("cuda", dt)
    B = (opB.t() if bk else opB).contiguous().to("cuda", dt)

    def path():
        plan = ext.gemm_plan(M, N, K, ak, bk, args.dtype == "bf16", True,
                             False)
        name = next((k for k in ("tr16", "tr16_nn", "split3") if plan[k]),
                    "generic")
        return (f"{name} {plan['bm']}x{plan['bn']} splitk {plan['splitk']} "
                f"kchunk {plan['kchunk']}")

    def measure(split):
        # correctness spot-check FIRST: the CPU reference matmul takes
        # seconds, and any GPU-idle gap right before the timed region lets
        # DVFS drop the clocks for the whole measurement (guide rule 24;
        # measured 50x once)
        if args.split:
            ext.set_fp32_split(split)
        out = ext.gemm(A, B, M, N, K, ak, bk)
        err = (out.cpu() - ref).abs().max().item()
        # clock ramp: keep the GPU busy ~100 ms right before timing
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.1:
            ext.gemm(A, B, M, N, K, ak, bk)
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            ext.gemm(A, B, M, N, K, ak, bk)
        torch.cuda.synchronize()
        dt_s = (time.perf_counter() - t0) / args.reps
        tf = 2.0 * M * N * K / dt_s / 1e12
        name = args.dtype + (" split" if split else "")
        print(f"{args.layout} {name} {M}x{N}x{K}: {tf:.1f} TF/s "
              f"({dt_s * 1e3:.3f} ms), max_err={err:.3g} [{path()}]")
        return dt_s

    ref = (opA.to(dt).float() @ opB.to(dt).float())
    was, was_nn = ext.fp32_split(), ext.tr16_nn()
    try:
        if args.nn_ab:
            ext.set_tr16_nn(False)
        exact = measure(False)
        if args.split:
            print(f"split / exact speed: {exact / measure(True):.2f}x")
        if args.nn_ab:
            ext.set_tr16_nn(True)
            print(f"tr16_nn / generic speed: {exact / measure(False):.2f}x")
    finally:
        ext.set_fp32_split(was)
        ext.set_tr16_nn(was_nn)


if __name__ == "__main__":
    main()
