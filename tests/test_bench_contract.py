"""bench.py output contract (the driver parses this JSON line)."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--model", "lenet",
         "--steps", "2", "--warmup", "1", "--no-graph"],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    rec = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in rec, key
    assert rec["metric"] == "images/sec (whole node)"
    assert rec["n_gpus"] == 1 and rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["higher_is_better"] is True
    assert rec["scaling"] == "weak"
    assert rec["data"] == "synthetic"
    assert rec["value"] > 0
    cfg = rec["config"]
    for key in ("model", "global_batch", "input", "parallelism"):
        assert key in cfg, key
    assert cfg["parallelism"] == "dp1"


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes float32 .npy arrays (loss, parameters,
    gradients) within the size budget, and two runs with the same arguments
    write the same files with the same shapes (bit-identical on CPU)."""
    import numpy as np

    def run(d):
        out = subprocess.run(
            [sys.executable, os.path.join(REPO, "bench.py"), "--model",
             "lenet", "--steps", "2", "--warmup", "1", "--no-graph",
             "--full", "--dump-outputs", str(d)],
            cwd=REPO, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        rec = json.loads([l for l in out.stdout.splitlines()
                          if l.startswith("{")][-1])
        assert rec["steps"] == 2 and rec["ms_per_step"] > 0
        return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}

    a, b = run(tmp_path / "a"), run(tmp_path / "b")
    assert list(a) == list(b)
    assert any(f.startswith("out_") for f in a)
    assert any(f.startswith("param_") for f in a)
    assert any(f.startswith("grad_") for f in a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    on_cpu = not __import__("torch").cuda.is_available()
    for f in a:
        assert a[f].dtype == np.float32, f
        assert a[f].shape == b[f].shape, f
        assert np.isfinite(a[f]).all(), f
        if on_cpu:  # GPU atomics reorder sums, so only CPU runs are bitwise
            assert np.array_equal(a[f], b[f]), f
