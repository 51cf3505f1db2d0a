"""Gather-GEMM address walk (row context once, taps by increment), checked on
the host: compiles tests/gather_walk_host.cpp (which includes ps_gather.h,
the header gemm.hip's staging and gather_addr compute addresses with) with
the host compiler and runs it -- once plain, once under AddressSanitizer +
UBSan. No GPU needed."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "poseidon_amd", "ops", "csrc")
SRC = os.path.join(HERE, "gather_walk_host.cpp")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _build_and_run(tmp_path, flags):
    assert CXX, "the extension build needs a host C++ compiler too"
    exe = str(tmp_path / "gather_walk_host")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    *flags, "-I", CSRC, SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all gather-walk host checks passed" in r.stdout


def test_walked_taps_and_offsets_equal_the_direct_decode(tmp_path):
    _build_and_run(tmp_path, [])


def test_gather_walk_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, ["-fsanitize=address,undefined",
                              "-fno-sanitize-recover=undefined"])
