"""Per-position ACCURACY and the two-top SOFTMAX_LOSS on the CPU, and the
two-tile plan of the softmax backward checked by a host program."""

import os
import shutil
import subprocess

import pytest
import torch

import poseidon_amd as pa
from poseidon_amd.core.net import Net, TRAIN
from poseidon_amd.ops import functional as ops
from poseidon_amd.proto import parse_text

HERE = os.path.dirname(os.path.abspath(__file__))


def sorted_hits(x, labels, top_k):
    """The reference's algorithm (accuracy_layer.cpp:46-66), position by
    position: sort (value, index) pairs descending, look for the label among
    the first top_k."""
    n, c, h, w = x.shape
    hits = 0
    for i in range(n):
        for y in range(h):
            for z in range(w):
                pairs = sorted(((x[i, k, y, z].item(), k) for k in range(c)),
                               reverse=True)
                label = int(labels[(i * h + y) * w + z])
                hits += label in [k for _, k in pairs[:top_k]]
    return hits


@pytest.mark.parametrize("top_k", [1, 2, 4])
def test_per_position_accuracy_is_the_sorted_top_k(top_k):
    g = torch.Generator().manual_seed(7)
    x = torch.randint(0, 3, (2, 4, 3, 3), generator=g).float()  # ties
    labels = torch.randint(0, 4, (18,), generator=g).float()
    labels[4], labels[9] = -1, 4  # no class: wrong, whatever top_k
    acc = ops.accuracy(x, labels, top_k)
    assert acc.shape == () and acc.dtype == torch.float32
    assert round(acc.item() * 18) == sorted_hits(x, labels, top_k)


def test_accuracy_rejects_other_label_counts_and_top_k_beyond_c():
    x = torch.zeros(2, 4, 3, 3)
    with pytest.raises(ValueError, match=r"2 labels.*or 18 .*got 6"):
        ops.accuracy(x, torch.zeros(6))
    with pytest.raises(ValueError, match="top_k = 5"):
        ops.accuracy(x, torch.zeros(18), 5)
    assert ops.accuracy(x, torch.zeros(2)).item() == 1.0  # one per image


_NET = """
    layers { name: "data" type: DUMMY_DATA top: "data" top: "label"
      dummy_data_param { num: 2 channels: 3 height: 6 width: 7
        num: 2 channels: 1 height: 6 width: 7
        data_filler { type: "gaussian" }
        data_filler { type: "uniform" min: 0 max: 2.99 } } }
    layers { name: "score" type: CONVOLUTION bottom: "data" top: "score"
      convolution_param { num_output: 3 kernel_size: 1
        weight_filler { type: "gaussian" std: 0.5 } } }
    layers { name: "loss" type: SOFTMAX_LOSS bottom: "score" bottom: "label"
      top: "loss" top: "prob" }
    layers { name: "acc" type: ACCURACY bottom: "prob" bottom: "label"
      top: "acc" accuracy_param { top_k: %d } }
    layers { name: "sm" type: SOFTMAX bottom: "score" top: "sm" }
    layers { name: "fit" type: EUCLIDEAN_LOSS bottom: "sm" bottom: "data"
      top: "fit" }
"""


def build(device="cpu", top_k=2):
    pa.init(device=device, seed=3, compute_dtype=torch.float32)
    return Net(parse_text("NetParameter", _NET % top_k), phase=TRAIN,
               verbose=False)


def test_softmax_loss_fills_a_second_top_that_feeds_accuracy():
    net = build()
    net.forward()
    net.zero_param_diffs()
    net.backward()
    prob, score = net.blobs["prob"], net.blobs["score"]
    layer = net.layers[net.layer_names.index("loss")]
    assert prob.shape == score.shape == (2, 3, 6, 7)
    assert prob.data.data_ptr() == layer._prob.data_ptr()
    assert torch.allclose(prob.data, torch.softmax(score.data, 1), atol=1e-6)
    labels = net.blobs["label"].data.reshape(-1)
    assert round(net.blobs["acc"].data.item() * 84) == \
        sorted_hits(prob.data, labels, 2)
    with pytest.raises(ValueError, match="top_k = 4"):
        build(top_k=4)


def test_two_tile_plan_on_the_host(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "the extension build needs a host C++ compiler too"
    exe = str(tmp_path / "softmax_heads_plan_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-D__host__=", "-D__device__=", "-I",
                    os.path.join(HERE, "..", "poseidon_amd", "ops", "csrc"),
                    os.path.join(HERE, "softmax_heads_plan_host.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all softmax-heads plan host checks passed" in r.stdout
