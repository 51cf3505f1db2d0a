"""Row-fused first-layer conv plan (tile walk, staged-row addressing, LDS
need, plan policy), checked on the host: compiles
tests/rowfused_plan_host.cpp (which includes ps_rowfused.h, the header
conv_rowfused.hip's kernels walk tiles and address staged rows with, and
ps_conv_plan.h) with the host compiler and runs it -- once plain, once under
AddressSanitizer + UBSan. No GPU needed."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "poseidon_amd", "ops", "csrc")
SRC = os.path.join(HERE, "rowfused_plan_host.cpp")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _build_and_run(tmp_path, flags):
    assert CXX, "the extension build needs a host C++ compiler too"
    exe = str(tmp_path / "rowfused_plan_host")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    *flags, "-I", CSRC, SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all row-fused plan host checks passed" in r.stdout


def test_tile_walk_addresses_and_lds_need(tmp_path):
    _build_and_run(tmp_path, [])


def test_rowfused_plan_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, ["-fsanitize=address,undefined",
                              "-fno-sanitize-recover=undefined"])
