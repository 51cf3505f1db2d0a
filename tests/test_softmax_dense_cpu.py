"""Dense (per-position) SOFTMAX_LOSS on the CPU: the two ops against the
float64 definition, and the layer's choice between the dense and the
classifier reading of its bottom."""

import pytest
import torch
import torch.nn.functional as F

import poseidon_amd as pa
from poseidon_amd.core.net import Net, TRAIN
from poseidon_amd.ops import functional as ops
from poseidon_amd.proto import parse_text


def reference(x, labels, w=1.0):
    """float64: log_softmax over dim 1, the label's term, mean over N*H*W."""
    n, c, h, wd = x.shape
    idx = labels.reshape(n, 1, h, wd).long()
    logp = F.log_softmax(x.double(), dim=1)
    onehot = torch.zeros_like(logp).scatter_(1, idx, 1.0)
    return (-logp.gather(1, idx).mean(), logp.exp(),
            (logp.exp() - onehot) * (w / idx.numel()))


@pytest.mark.parametrize("shape", [(2, 2, 3, 5), (1, 21, 7, 9), (3, 5, 1, 4)])
def test_ops_match_the_definition(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g) * 4
    n, c, h, w = shape
    labels = torch.randint(0, c, (n * h * w,), generator=g).float()
    ref_loss, ref_prob, ref_dx = reference(x, labels, 0.7)
    loss, prob = ops.softmax_loss_forward(x, labels)
    dx = ops.softmax_loss_backward(prob, labels, 0.7)
    assert prob.shape == x.shape and dx.shape == x.shape
    assert abs(loss.item() - ref_loss.item()) <= 2e-4 * max(1.0, ref_loss)
    assert (prob.double() - ref_prob).abs().max() <= 2e-4
    assert (dx.double() - ref_dx).abs().max() <= 2e-4
    with pytest.raises(ValueError, match="labels"):
        ops.softmax_loss_forward(x, labels[:n])


def test_max_c_mirror_matches_the_plan():
    if ops.ext_available():
        assert ops._ext().softmax_dense_max_c() == ops.SOFTMAX_DENSE_MAX_C


_NET = """
    layers { name: "data" type: DUMMY_DATA top: "data" top: "label"
      dummy_data_param { num: 2 channels: 3 height: 6 width: 7
        num: 2 channels: 1 height: %d width: %d
        data_filler { type: "gaussian" }
        data_filler { type: "uniform" min: 0 max: 4.99 } } }
    layers { name: "score" type: CONVOLUTION bottom: "data" top: "score"
      convolution_param { num_output: 5 kernel_size: 1
        weight_filler { type: "gaussian" std: 0.5 } } }
    layers { name: "loss" type: SOFTMAX_LOSS bottom: "score" bottom: "label"
      top: "loss" }
"""


def build(lh, lw):
    pa.init(device="cpu", seed=3, compute_dtype=torch.float32)
    return Net(parse_text("NetParameter", _NET % (lh, lw)), phase=TRAIN,
               verbose=False)


def test_layer_takes_the_dense_path_for_per_position_labels():
    net = build(6, 7)
    loss = net.forward()
    net.zero_param_diffs()
    net.backward()
    score, labels = net.blobs["score"], net.blobs["label"].data
    ref_loss, _, ref_dx = reference(score.data, labels)
    assert abs(loss - ref_loss.item()) <= 2e-4 * max(1.0, ref_loss)
    assert (score.diff.double() - ref_dx).abs().max() <= 2e-4


def test_layer_keeps_the_classifier_path_for_per_image_labels():
    net = build(1, 1)
    loss = net.forward()
    score, labels = net.blobs["score"], net.blobs["label"].data
    flat, _ = ops.softmax_loss_forward(score.data.reshape(2, -1),
                                       labels.reshape(-1))
    assert loss == flat.item()


def test_layer_rejects_any_other_label_count():
    with pytest.raises(ValueError, match=r"\(2, 5, 6, 7\).*\(2, 1, 3, 7\)"):
        build(3, 7)
