"""Blob-statistics planner checked on the host: compiles
tests/stats_plan_host.cpp (which includes ps_stats_plan.h, the header
stats.hip launches from) with the host compiler and runs it -- once plain,
once under AddressSanitizer + UBSan. No GPU needed."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "poseidon_amd", "ops", "csrc")
SRC = os.path.join(HERE, "stats_plan_host.cpp")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _build_and_run(tmp_path, flags):
    assert CXX, "the extension build needs a host C++ compiler too"
    exe = str(tmp_path / "stats_plan_host")
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    *flags, "-I", CSRC, SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all stats-plan host checks passed" in r.stdout


def test_plan_covers_every_element_once_within_its_chain(tmp_path):
    _build_and_run(tmp_path, [])


def test_plan_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, ["-fsanitize=address,undefined",
                              "-fno-sanitize-recover=undefined"])
