"""Packed first-layer conv layout, checked on the host: compiles
tests/packed_conv_host.cpp (which includes ps_conv_plan.h, the header the
kernels and the bindings use) with the host compiler and runs it -- once
plain, once under AddressSanitizer + UBSan. No GPU needed."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "poseidon_amd", "ops", "csrc")
SRC = os.path.join(HERE, "packed_conv_host.cpp")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _build_and_run(tmp_path, flags):
    assert CXX, "the extension build needs a host C++ compiler too"
    exe = str(tmp_path / "packed_conv_host")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    *flags, "-I", CSRC, SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all packed-conv host checks passed" in r.stdout


def test_packed_layout_matches_direct_conv(tmp_path):
    _build_and_run(tmp_path, [])


def test_packed_layout_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, ["-fsanitize=address,undefined",
                              "-fno-sanitize-recover=undefined"])
