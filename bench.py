#!/usr/bin/env python3
"""Flagship benchmark: whole-node images/sec for AlexNet (default) /
GoogLeNet / VGG-16 / CIFAR-quick on synthetic data with random-init weights
(BASELINE.json metric). One rank per GPU over RCCL; launch N>1 via
torch.distributed.run with --master-addr 127.0.0.1.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \
        --master-addr 127.0.0.1 bench.py --gpus 8 --steps 20 --warmup 5

A plain run sets up, warms up, times --steps iterations and prints one JSON
line. --dump-outputs DIR additionally writes what the last timed iteration
left behind (net outputs, updated parameters and their gradients) as
DIR/<name>.npy so two builds can be compared array for array; that iteration
then starts from the seeded initial weights, so the arrays do not depend on
run-to-run rounding noise accumulated over the earlier steps. --full is
reserved for measurements beyond the headline figure; there are none at
present, so it changes nothing.
"""

import argparse
import json
import os
import time

import torch


DEFAULT_BATCH = {  # per-GPU batch, matching the reference's training configs
    "alexnet": 256,   # models/bvlc_alexnet/train_val.prototxt:10
    "caffenet": 256,  # models/bvlc_reference_caffenet/train_val.prototxt
    "googlenet": 32,  # models/bvlc_googlenet/train_test.prototxt:9
    "vgg16": 32,
    "cifar10_quick": 100,
    "lenet": 64,
}

DUMP_BUDGET_BYTES = 32 << 20  # all .npy files together stay under this
DUMP_SAMPLE_SEED = 20240


def dump_outputs(solver, out_dir):
    """Write the arrays the last solver iteration produced as float32 .npy:
    out_<blob> (net outputs, i.e. the loss), param_<i>_<name> (weights
    after the update) and grad_<i>_<name> (the gradients that update
    consumed) -- what a caller of solver.step() is left holding.
    main() starts that iteration from the seeded initial weights, so the
    arrays are one full step (forward, backward, update) of those weights.
    Arrays larger than an equal share of DUMP_BUDGET_BYTES are reduced to a
    fixed, seeded sample of their elements (same indices every run)."""
    import numpy as np

    arrays = []
    for name in sorted(solver.net.output_blob_names):
        arrays.append((f"out_{name}", solver.net.blobs[name].data))
    for i, ps in enumerate(solver.net.params):
        if ps.owner != i:
            continue
        arrays.append((f"param_{i}_{ps.blob.name}", ps.blob.data))
        if ps.blob.has_diff():
            arrays.append((f"grad_{i}_{ps.blob.name}", ps.blob.diff))
    cap = max(1, DUMP_BUDGET_BYTES // 4 // len(arrays))
    os.makedirs(out_dir, exist_ok=True)
    for k, (name, t) in enumerate(arrays):
        flat = t.detach().reshape(-1)
        if flat.numel() > cap:
            g = torch.Generator().manual_seed(DUMP_SAMPLE_SEED + k)
            idx = torch.randint(0, flat.numel(), (cap,), generator=g)
            flat = flat[idx.sort().values.to(flat.device)]
            arr = flat.to(torch.float32).cpu().numpy()
        else:
            arr = t.detach().to(torch.float32).cpu().numpy()
        fname = "".join(c if c.isalnum() or c in "._-" else "_" for c in name)
        np.save(os.path.join(out_dir, fname + ".npy"), arr)


def rewind(solver, start_state):
    """Put the owned parameters back to start_state and clear the momentum
    history, in place (tensor identities, and so the captured graph and the
    multi-tensor tables, stay valid)."""
    owned = [ps for i, ps in enumerate(solver.net.params) if ps.owner == i]
    for ps, w0 in zip(owned, start_state):
        ps.blob.data.copy_(w0)
    for h in solver.history.values():
        h.zero_()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--model", default="alexnet",
                    choices=list(DEFAULT_BATCH))
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch")
    ap.add_argument("--no-sfb", action="store_true")
    ap.add_argument("--implicit", action="store_true",
                    help="implicit-GEMM convolutions (gather in GEMM staging"
                         " instead of materialized im2col)")
    ap.add_argument("--no-graph", action="store_true",
                    help="disable hipGraph capture of the iteration")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"],
                    help="compute dtype (activations + GEMM inputs); "
                         "master weights and gradient accumulation stay fp32")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write the last step's "
                         "outputs, updated parameters and gradients to "
                         "DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run measurements beyond the headline figure "
                         "(none at present)")
    args = ap.parse_args()

    import poseidon_amd as pa
    from poseidon_amd.models import zoo
    from poseidon_amd.proto import Message
    from poseidon_amd.solver.solver import SGDSolver
    from poseidon_amd.parallel import comm

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    assert world == args.gpus or args.gpus == 1 or world == 1, \
        f"WORLD_SIZE={world} vs --gpus={args.gpus}"
    n_gpus = max(world, 1)

    device = "cuda" if torch.cuda.is_available() else "cpu"
    cd = torch.bfloat16 if (args.dtype == "bf16" and device == "cuda") \
        else torch.float32
    pa.init(device=device, seed=1234, compute_dtype=cd)
    if args.implicit and device == "cuda":
        from poseidon_amd.ops import functional as F
        F.set_implicit_gemm(True)
    batch = args.batch or DEFAULT_BATCH[args.model]

    sp = Message("SolverParameter", base_lr=0.01, lr_policy="fixed",
                 momentum=0.9, weight_decay=0.0005, max_iter=1 << 30,
                 display=0, snapshot=0)
    sp.net_param = zoo.build_net(args.model, batch=batch)
    solver = SGDSolver(sp, use_sfb=not args.no_sfb, verbose=False)
    graphed = False
    if not args.no_graph and device == "cuda":
        # RCCL collectives are hipGraph-capturable: the multi-rank graph
        # replays DWBP all-reduces + SFB all-gathers in-graph; capture
        # success is agreed across ranks and falls back to eager everywhere
        # if any rank fails (solver._capture_graph). PS_GRAPH=0 disables.
        if os.environ.get("PS_GRAPH", "1") != "0":
            graphed = solver.enable_graph()

    start_state = None
    if args.dump_outputs:
        assert args.steps >= 1, "--dump-outputs needs at least one timed step"
        start_state = [ps.blob.data.clone()
                       for i, ps in enumerate(solver.net.params)
                       if ps.owner == i]

    def sync():
        if device == "cuda":
            torch.cuda.synchronize()
        comm.barrier()

    solver.step(args.warmup)
    # report the truth: capture may have fallen back to eager during warmup
    graphed = bool(solver._use_graph and solver._graph is not None)
    sync()
    t0 = time.perf_counter()
    if start_state is None:
        solver.step(args.steps)
        sync()
        elapsed = time.perf_counter() - t0
    else:
        # Split-K atomics make every step's gradients differ in the last
        # bits from run to run, and training amplifies that over the steps.
        # So that the dumped arrays depend only on the seed, the last timed
        # step starts from the seeded initial weights and zero momentum;
        # the rewind itself is kept off the clock.
        solver.step(args.steps - 1)
        sync()
        elapsed = time.perf_counter() - t0
        rewind(solver, start_state)
        sync()
        t0 = time.perf_counter()
        solver.step(1)
        sync()
        elapsed += time.perf_counter() - t0

    # MAX elapsed over ranks (staged through the device for nccl/RCCL)
    t = torch.tensor([elapsed], dtype=torch.float64)
    if solver.distributed:
        comm.allreduce_max(t)
    elapsed = float(t[0])

    if args.dump_outputs and rank == 0:
        dump_outputs(solver, args.dump_outputs)

    if rank == 0:
        images = batch * n_gpus * args.steps
        value = images / elapsed
        out = {
            "metric": "images/sec (whole node)",
            "value": round(value, 2),
            "unit": "images/sec",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype if device == "cuda" else "fp32",
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": batch * n_gpus,
                "input": {"alexnet": "3x227x227", "caffenet": "3x227x227",
                          "googlenet": "3x224x224",
                          "vgg16": "3x224x224", "cifar10_quick": "3x32x32",
                          "lenet": "1x28x28"}[args.model],
                "parallelism": f"dp{n_gpus}",
                "sfb": not args.no_sfb and n_gpus > 1,
                "hipgraph": graphed,
            },
        }
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
