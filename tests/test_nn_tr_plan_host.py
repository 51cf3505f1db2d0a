"""NN tr16 plans (ps_gemm_plan.h, ps_nn_tr_plan), checked on the host:
compiles tests/nn_tr_plan_host.cpp with the host compiler and runs it, plain
and under AddressSanitizer + UBSan. No GPU needed."""

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "poseidon_amd", "ops", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "sanitizers"])
def test_nn_tr_plans_hold_the_kernel_invariants(tmp_path, flags):
    assert CXX, "the extension build needs a host C++ compiler too"
    exe = str(tmp_path / "nn_tr_plan_host")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags,
                    "-I", CSRC, os.path.join(HERE, "nn_tr_plan_host.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host checks passed" in r.stdout, \
        r.stdout[-4000:] + r.stderr[-4000:]
