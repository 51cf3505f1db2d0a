"""Solver debug_info on the CPU path: which iterations report, the
reference's line format and order (net.cpp:787-852), the record values
against tensors the test snapshots itself, and that the switch changes
nothing about training.

The net is conv -> in-place relu -> pool -> ip1 -> ip2 -> ip3 -> softmax
loss; ip2 shares ip1's two named params."""

import re

import pytest
import torch

import poseidon_amd as pa
from poseidon_amd.proto import Message, parse_text
from poseidon_amd.solver.solver import (AdaGradSolver, NesterovSolver,
                                        SGDSolver)

_NET = """
    name: "dbgnet"
    layers { name: "data" type: DUMMY_DATA top: "data" top: "label"
             dummy_data_param { num: 4 channels: 2 height: 6 width: 6
                 num: 4 channels: 1 height: 1 width: 1
                 data_filler { type: "gaussian" std: 1.0 }
                 data_filler { type: "constant" } } }
    layers { name: "conv1" type: CONVOLUTION bottom: "data" top: "conv1"
             blobs_lr: 1 blobs_lr: 2
             convolution_param { num_output: 4 kernel_size: 3 pad: 1
                 weight_filler { type: "gaussian" std: 0.3 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "relu1" type: RELU bottom: "conv1" top: "conv1" }
    layers { name: "pool1" type: POOLING bottom: "conv1" top: "pool1"
             pooling_param { pool: MAX kernel_size: 2 stride: 2 } }
    layers { name: "ip1" type: INNER_PRODUCT bottom: "pool1" top: "ip1"
             param: "w" param: "b" blobs_lr: 1 blobs_lr: 2
             inner_product_param { num_output: 36
                 weight_filler { type: "gaussian" std: 0.2 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "ip2" type: INNER_PRODUCT bottom: "ip1" top: "ip2"
             param: "w" param: "b" blobs_lr: 1 blobs_lr: 2
             inner_product_param { num_output: 36
                 weight_filler { type: "gaussian" std: 0.2 }
                 bias_filler { type: "constant" value: 0.1 } } }
    layers { name: "ip3" type: INNER_PRODUCT bottom: "ip2" top: "ip3"
             blobs_lr: 1 blobs_lr: 2
             inner_product_param { num_output: 5
                 weight_filler { type: "gaussian" std: 0.2 }
                 bias_filler { type: "constant" } } }
    layers { name: "loss" type: SOFTMAX_LOSS bottom: "ip3" bottom: "label"
             top: "loss" }
"""

# the reference's lines for this net, values cut off, in its order
_FORWARD = [f"    [Forward] Layer {l}, top blob {t} data: " for l, t in (
    ("data", "data"), ("data", "label"), ("conv1", "conv1"),
    ("relu1", "conv1"), ("pool1", "pool1"), ("ip1", "ip1"), ("ip2", "ip2"),
    ("ip3", "ip3"), ("loss", "loss"))]
_BACKWARD = [f"    [Backward] Layer {l}, {w} diff: " for l, w in (
    ("loss", "bottom blob ip3"),
    ("ip3", "bottom blob ip2"), ("ip3", "param blob 0"),
    ("ip3", "param blob 1"),
    ("ip2", "bottom blob ip1"), ("ip2", "param blob 0"),
    ("ip2", "param blob 1"),
    ("ip1", "bottom blob pool1"), ("ip1", "param blob 0"),
    ("ip1", "param blob 1"),
    ("pool1", "bottom blob conv1"), ("relu1", "bottom blob conv1"),
    ("conv1", "param blob 0"), ("conv1", "param blob 1"))]
_UPDATE = [
    "    [Update] Layer conv1, param 0 data: ",
    "    [Update] Layer conv1, param 1 data: ",
    "    [Update] Layer ip1, param w data: ",
    "    [Update] Layer ip1, param b data: ",
    "    [Update] Layer ip2, param blob w (owned by layer ip1, param w) diff: ",
    "    [Update] Layer ip2, param blob b (owned by layer ip1, param b) diff: ",
    "    [Update] Layer ip3, param 0 data: ",
    "    [Update] Layer ip3, param 1 data: ",
]
_NUM = r"(?:-?\d+(?:\.\d+)?(?:e[+-]\d+)?|inf|nan)"
_LINE = re.compile(
    r"^    \[(?:Forward\] Layer \S+, top blob \S+ data: " + _NUM +
    r"|Backward\] Layer \S+, (?:bottom blob \S+|param blob \d+) diff: " +
    _NUM +
    r"|Update\] Layer \S+, param \S+ data: " + _NUM + "; diff: " + _NUM +
    r"|Update\] Layer \S+, param blob \S+ \(owned by layer \S+, param \S+\)"
    r" diff: " + _NUM + r")$")


def _solver(cls=SGDSolver, debug=True, verbose=True, display=2):
    pa.init(device="cpu", seed=11, compute_dtype=torch.float32)
    sp = Message("SolverParameter", base_lr=0.05, lr_policy="fixed",
                 momentum=0.9, weight_decay=0.001, max_iter=100,
                 display=display, snapshot=0, debug_info=debug)
    if cls is AdaGradSolver:
        sp.momentum = 0.0
        sp.delta = 1e-8
    sp.net_param = parse_text("NetParameter", _NET)
    return cls(sp, verbose=verbose)


def _debug_lines(text):
    return [l for l in text.splitlines()
            if l.startswith("    [") and not l.startswith("    [Watch]")]


def test_only_display_iterations_print(capsys):
    s = _solver()
    s.step(6)
    lines = capsys.readouterr().out.splitlines()
    per_iter = len(_FORWARD) + len(_BACKWARD) + len(_UPDATE)
    shown = [i for i, l in enumerate(lines) if l.startswith("[poseidon] iter")]
    assert [lines[i].split()[2] for i in shown] == ["0", "2", "4"]
    assert len(_debug_lines("\n".join(lines))) == 3 * per_iter
    for i in shown:  # each block sits right before its display line
        block = lines[i - per_iter:i]
        assert all(l.startswith("    [") for l in block)

    s = _solver(debug=False)
    s.step(6)
    out = capsys.readouterr().out
    assert "[poseidon] iter 4" in out and not _debug_lines(out)
    assert s.debug_records == []


def test_line_format_and_order(capsys):
    s = _solver()
    s.step(1)
    lines = _debug_lines(capsys.readouterr().out)
    want = _FORWARD + _BACKWARD + _UPDATE
    assert len(lines) == len(want)
    for line, prefix in zip(lines, want):
        assert _LINE.match(line), line
        assert line.startswith(prefix), (line, prefix)


def _mean(t):
    return float(t.detach().abs().double().mean())


def _snapshot_step(s):
    """One step with layer.forward / layer.backward / net.backward wrapped:
    the mean |x| of every top as its forward returns, of every gradient-
    carrying bottom diff as its backward returns, and of the params' diffs
    and data when backward is through. Keyed like the records."""
    net, snap, params = s.net, {}, {}
    lps = net.param.layers

    def wrap(i, layer):
        fwd, bwd = layer.forward, layer.backward

        def forward(bottom, top):
            fwd(bottom, top)
            for ti, t in enumerate(top):
                snap["forward", layer.name, "top", lps[i].top[ti]] = \
                    (_mean(t.data), int((~torch.isfinite(t.data)).sum()))

        def backward(top, propagate_down, bottom):
            bwd(top, propagate_down, bottom)
            for j, b in enumerate(bottom):
                if propagate_down[j]:
                    snap["backward", layer.name, "bottom",
                         lps[i].bottom[j]] = (_mean(b.diff), 0)
        layer.forward, layer.backward = forward, backward
        return fwd, bwd

    saved = [wrap(i, l) for i, l in enumerate(net.layers)]
    net_bwd = net.backward

    def backward(*a, **k):
        net_bwd(*a, **k)
        for idx, ps in enumerate(net.params):
            params[idx] = (_mean(ps.blob.diff), _mean(ps.blob.data),
                           ps.blob.data.detach().clone())
    net.backward = backward
    try:
        s.step(1)
    finally:
        del net.backward
        for l, (fwd, bwd) in zip(net.layers, saved):
            del l.forward, l.backward
    return snap, params


@pytest.mark.parametrize("cls", [SGDSolver, NesterovSolver, AdaGradSolver])
def test_record_values(cls):
    s = _solver(cls, verbose=False)
    snap, params = _snapshot_step(s)
    recs = s.debug_records
    assert len(recs) == len(_FORWARD) + len(_BACKWARD) + len(_UPDATE)
    assert all(r["available"] for r in recs)
    net = s.net
    idx_of = {(net.layers[ps.layer_idx].name, ps.param_idx): i
              for i, ps in enumerate(net.params)}
    seen = 0
    for r in recs:
        if r["phase"] == "update":
            i = idx_of[r["layer"], r["param_idx"]]
            own = net.params[i].owner
            if cls is SGDSolver:
                want = _mean(s.history[own])
            else:
                want = _mean(params[own][2] - net.params[own].blob.data)
            assert r["mean_abs"] == want, r
            assert want > 0
            if own == i:
                assert r["data_mean_abs"] == params[i][1], r
                assert r["owner"] is None
            else:
                assert r["owner"] == ("ip1", "wb"[r["param_idx"]])
        elif r["kind"] == "param":
            i = idx_of[r["layer"], r["param_idx"]]
            assert r["mean_abs"] == params[i][0] and r["mean_abs"] > 0, r
        else:
            want, nf = snap[r["phase"], r["layer"], r["kind"], r["name"]]
            assert r["mean_abs"] == want and r["nonfinite"] == nf, r
            assert r["count"] > 0
            seen += 1
    # every snapshot was compared: tops, and the bottoms that need a gradient
    assert seen == len(snap) == len(_FORWARD) + 6


def test_training_is_unchanged():
    finals = []
    for debug in (True, False):
        s = _solver(debug=debug, verbose=False)
        s.step(6)
        finals.append([ps.blob.data.clone() for ps in s.net.params])
    for a, b in zip(*finals):
        assert torch.equal(a, b)


def test_overflow_watch(capsys):
    s = _solver()
    s.net.params[0].blob.data.view(-1)[0] = float("inf")
    s.step(1)
    out = capsys.readouterr().out.splitlines()
    watch = [l for l in out if l.startswith("    [Watch]")]
    top = s.net.blobs["conv1"].data
    bad = int((~torch.isfinite(top)).sum())
    assert 0 < bad < top.numel()
    finite = top[torch.isfinite(top)].abs().max()
    assert watch and watch[0] == (
        f"    [Watch] Layer conv1, top conv1: {bad} non-finite of "
        f"{top.numel()}, max finite |x| {'%g' % float(finite)}")
    # the watch lines follow the reference's lines, before the display line
    first = out.index(watch[0])
    assert all(l.startswith("    [") and not l.startswith("    [Watch]")
               for l in out[:first] if l.startswith("    "))
    assert out[-1].startswith("[poseidon] iter 0")
    rec = next(r for r in s.debug_records if r["nonfinite"])
    assert (rec["layer"], rec["kind"], rec["nonfinite"]) == \
        ("conv1", "top", bad)
