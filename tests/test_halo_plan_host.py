"""Halo-tile conv plan (tile coverage, patch staging and fragment reads, LDS
budget, channel order, eligibility), checked on the host: compiles
tests/halo_plan_host.cpp (which includes ps_halo.h, the header
conv_halo.hip's kernel walks and addresses with) with the host compiler and
runs it. No GPU needed."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "poseidon_amd", "ops", "csrc")
SRC = os.path.join(HERE, "halo_plan_host.cpp")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def test_halo_plan_on_the_host(tmp_path):
    assert CXX, "the extension build needs a host C++ compiler too"
    exe = str(tmp_path / "halo_plan_host")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, SRC,
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all halo plan host checks passed" in r.stdout
