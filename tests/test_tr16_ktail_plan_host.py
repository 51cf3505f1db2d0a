"""tr16 K-tail plans (K % 64 != 0 on the transpose-read TN kernel), checked
on the host: compiles tests/tr16_ktail_plan_host.cpp (which includes
ps_gemm_plan.h, the header gemm.hip plans and launches from) with the host
compiler and runs it. No GPU needed."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "poseidon_amd", "ops", "csrc")
SRC = os.path.join(HERE, "tr16_ktail_plan_host.cpp")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def test_ktail_plans_hold_the_slice_invariants(tmp_path):
    assert CXX, "the extension build needs a host C++ compiler too"
    exe = str(tmp_path / "tr16_ktail_plan_host")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, SRC,
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all tr16 K-tail plan checks passed" in r.stdout
