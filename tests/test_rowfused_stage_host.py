"""Row-fused conv window staging (which load fetches each 16 B vector of a
tile's staged image, what it may touch, what the register mask leaves),
checked on the host: compiles tests/rowfused_stage_host.cpp (which includes
ps_rowfused.h, the header conv_rowfused.hip's kernels decide, address and
mask with) with the host compiler and runs it -- once plain, once under
AddressSanitizer + UBSan. No GPU needed."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "poseidon_amd", "ops", "csrc")
SRC = os.path.join(HERE, "rowfused_stage_host.cpp")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _build_and_run(tmp_path, flags):
    assert CXX, "the extension build needs a host C++ compiler too"
    exe = str(tmp_path / "rowfused_stage_host")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    *flags, "-I", CSRC, SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all row-fused staging host checks passed" in r.stdout


def test_vector_kinds_bounds_and_window(tmp_path):
    _build_and_run(tmp_path, [])


def test_rowfused_staging_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, ["-fsanitize=address,undefined",
                              "-fno-sanitize-recover=undefined"])
