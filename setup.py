"""Build the in-tree HIP/CDNA4 extension for gfx950 (MI355X).

    PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace

The .so lands in poseidon_amd/ops/ (in-tree, so it travels to GPU boxes
with the repo snapshot)."""

import os

os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")

from setuptools import setup
from torch.utils.cpp_extension import BuildExtension, CUDAExtension

CSRC = os.path.join("poseidon_amd", "ops", "csrc")

sources = [
    os.path.join(CSRC, f)
    for f in [
        "bindings.cpp",
        "gemm.hip",
        "elementwise.hip",
        "pool.hip",
        "lrn.hip",
        "softmax.hip",
        "sgd.hip",
        "im2col.hip",
        "conv_rowfused.hip",
        "transform.hip",
        "stats.hip",
    ]
]

# Sanitizer preset (host side): PS_SANITIZE=address adds ASan to the C++
# binding layer -- a deliberate improvement over the reference, which had
# no sanitizer story (concurrency safety there was
# by-construction mutexes). Device code relies on numerics tests +
# compute-sanitizer-style tools where available.
_cxx = ["-O3"]
_ld = []
if os.environ.get("PS_SANITIZE") == "address":
    _cxx += ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"]
    _ld += ["-fsanitize=address"]
elif os.environ.get("PS_SANITIZE") == "thread":
    # TSAN for the host-side binding code (the HIP device code is outside
    # TSAN's scope; python-thread handoffs are covered by the prefetch
    # stress test instead, tests/test_prefetch_stress.py)
    _cxx += ["-fsanitize=thread", "-fno-omit-frame-pointer", "-g"]
    _ld += ["-fsanitize=thread"]

setup(
    name="poseidon_amd_hip",
    ext_modules=[
        CUDAExtension(
            name="poseidon_amd.ops._hip",
            sources=sources,
            extra_compile_args={
                "cxx": _cxx,
                "nvcc": ["-O3", "-std=c++17"],
            },
            extra_link_args=_ld,
        )
    ],
    cmdclass={"build_ext": BuildExtension},
)
