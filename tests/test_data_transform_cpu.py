"""Device-transform path of the DATA layer without a GPU: DataTransformer's
draw() + ops.data_transform (the torch CPU op, the numerics reference of the
HIP kernel) against the transformer's numpy __call__, and the layer with the
switch on against the layer with it off. Everything is compared for equality:
both sides do one fp32 subtract and one fp32 multiply per element."""

import numpy as np
import pytest
import torch

import poseidon_amd as pa
from poseidon_amd.core.net import Net, TRAIN, TEST
from poseidon_amd.data.pdb import PDBReader, datum_to_array
from poseidon_amd.data.transformer import DataTransformer
from poseidon_amd.ops import functional as ops
from poseidon_amd.proto import Message, parse_text

from data_transform_util import data_layer_text, write_mean, write_pdb

C, H, W = 3, 9, 11


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("dt")
    recs = write_pdb(d / "u8.pdb", 10, C, H, W)
    write_pdb(d / "f32.pdb", 10, C, H, W, float_data=True)
    write_pdb(d / "fifty.pdb", 50, C, H, W, seed=6)
    mean = write_mean(d / "mean.binaryproto", C, H, W)
    return {"dir": d, "recs": recs, "mean": mean}


def _configs(meanfile):
    return {
        "plain": "",
        "crop_mirror": "crop_size: 5 mirror: true",
        "mirror_only_scale": "mirror: true scale: 0.00390625",
        "meanfile_all": f'crop_size: 5 mirror: true mean_file: "{meanfile}" '
                        "scale: 0.017",
        "mean_scalar": "mean_value: 117.5 mirror: true scale: 0.017",
        "mean_channel": "mean_value: 104.25 mean_value: 116.7 "
                        "mean_value: 122.9 crop_size: 7",
    }


@pytest.mark.parametrize("phase", [TRAIN, TEST])
@pytest.mark.parametrize("cfg", ["plain", "crop_mirror", "mirror_only_scale",
                                 "meanfile_all", "mean_scalar",
                                 "mean_channel"])
def test_draw_plus_apply_equals_call(files, cfg, phase):
    text = _configs(files["dir"] / "mean.binaryproto")[cfg]
    tp = parse_text("TransformationParameter", text)
    old = DataTransformer(tp, phase, np.random.default_rng(77))
    new = DataTransformer(tp, phase, np.random.default_rng(77))
    mode, mean, scale, crop = new.device_spec(C, H, W)
    ho, wo = (crop, crop) if crop else (H, W)
    db = PDBReader(str(files["dir"] / "fifty.pdb"))
    assert len(db) == 50
    flips = 0
    for i in range(50):
        d = db.get(i)
        want = old(datum_to_array(d))
        h_off, w_off, flip = new.draw(H, W)
        flips += flip
        raw = torch.from_numpy(
            np.frombuffer(d.data, dtype=np.uint8).reshape(1, C, H, W).copy())
        params = torch.tensor([[h_off, w_off, flip]], dtype=torch.int32)
        out = torch.full((1, C, ho, wo), -7.0)
        ops.data_transform(raw, params, mean, mode, scale, out)
        assert want.dtype == np.float32 and want.shape == (C, ho, wo)
        assert np.array_equal(out[0].numpy(), want), f"image {i}"
    if "mirror" in text and phase == TRAIN:
        assert 0 < flips < 50
    else:
        assert flips == 0
    # both generators were consumed alike
    assert old.rng.integers(0, 1 << 30) == new.rng.integers(0, 1 << 30)


def test_device_spec_rejects_a_mean_image_of_another_shape(files):
    tp = parse_text("TransformationParameter",
                    f'mean_file: "{files["dir"] / "mean.binaryproto"}"')
    t = DataTransformer(tp, TRAIN, np.random.default_rng(1))
    with pytest.raises(ValueError, match="mean image"):
        t.device_spec(C, H + 1, W)


def _forwards(pdb, transform, switch, n=6, seed=11):
    """n forwards of a batch-4 DATA net; returns ([data], [label], ids of
    the data top's tensor, layer)."""
    pa.init(device="cpu", seed=seed, compute_dtype=torch.float32,
            device_transform=switch)
    try:
        net = Net(parse_text("NetParameter", 'name: "dt"'
                             + data_layer_text(pdb, 4, transform)),
                  phase=TRAIN, verbose=False)
        datas, labels, tensors = [], [], []
        for _ in range(n):
            net.forward()
            tensors.append(net.blobs["data"].data)
            datas.append(net.blobs["data"].data.clone())
            labels.append(net.blobs["label"].data.clone())
        return datas, labels, tensors, net.layers[0]
    finally:
        pa.init(device="cpu", device_transform=False)


def _full_transform(files):
    return (f'crop_size: 5 mirror: true scale: 0.017 '
            f'mean_file: "{files["dir"] / "mean.binaryproto"}"')


def test_layer_switch_on_equals_switch_off(files):
    """10 records, batch 4: the cursor wraps in the middle of the third
    batch. Same context seed, so the same crops and mirrors."""
    pdb = files["dir"] / "u8.pdb"
    off = _forwards(pdb, _full_transform(files), False)
    on = _forwards(pdb, _full_transform(files), True)
    assert not off[3].on_device and on[3].on_device
    for k in range(6):
        assert on[0][k].shape == (4, C, 5, 5)
        assert on[0][k].dtype == off[0][k].dtype == torch.float32
        assert torch.equal(on[0][k], off[0][k]), f"data, forward {k}"
        assert torch.equal(on[1][k], off[1][k]), f"label, forward {k}"
        assert on[1][k].dtype == off[1][k].dtype
    # labels are i % 5 over 10 records: the wrap shows in the third batch
    assert off[1][2].tolist() == [3.0, 4.0, 0.0, 1.0]
    assert not torch.equal(off[0][0], off[0][1])
    # the device path writes into one persistent top
    assert all(t is on[2][0] for t in on[2])


def test_float_data_records_keep_the_host_path(files):
    pdb = files["dir"] / "f32.pdb"
    off = _forwards(pdb, _full_transform(files), False)
    on = _forwards(pdb, _full_transform(files), True)
    assert not on[3].on_device
    for k in range(6):
        assert torch.equal(on[0][k], off[0][k])
        assert torch.equal(on[1][k], off[1][k])
    # and it is the same data the uint8 file gives
    u8 = _forwards(files["dir"] / "u8.pdb", _full_transform(files), True)
    assert torch.equal(u8[0][5], on[0][5])


def test_a_float_record_met_later_raises(files, tmp_path):
    """First record uint8 (device path taken), a later one float_data."""
    from poseidon_amd.data.pdb import PDBWriter, array_to_datum
    path = tmp_path / "mixed.pdb"
    with PDBWriter(str(path)) as wtr:
        for i, r in enumerate(files["recs"][:6]):
            wtr.put(array_to_datum(r if i != 5 else r.astype(np.float32), i))
    with pytest.raises(ValueError, match="float_data record"):
        _forwards(path, "crop_size: 5", True, n=2)


def test_a_record_of_another_shape_raises(files, tmp_path):
    from poseidon_amd.data.pdb import PDBWriter, array_to_datum
    path = tmp_path / "shapes.pdb"
    with PDBWriter(str(path)) as wtr:
        for i, r in enumerate(files["recs"][:6]):
            wtr.put(array_to_datum(r if i != 4 else r[:, :8, :].copy(), i))
    with pytest.raises(ValueError, match="device-transform path"):
        _forwards(path, "crop_size: 5", True, n=2)


def test_switch_defaults_off_and_gating_is_untouched(files):
    assert pa.ctx().device_transform is False
    from poseidon_amd.solver.solver import SGDSolver
    pa.init(device="cpu", seed=3, compute_dtype=torch.float32)
    sp = Message("SolverParameter", base_lr=0.01, lr_policy="fixed",
                 max_iter=10, display=0, snapshot=0)
    sp.net_param = parse_text("NetParameter", 'name: "g"' + data_layer_text(
        files["dir"] / "u8.pdb", 4, "crop_size: 5") + """
        layers { name: "ip" type: INNER_PRODUCT bottom: "data" top: "ip"
                 inner_product_param { num_output: 5
                     weight_filler { type: "gaussian" std: 0.1 } } }
        layers { name: "loss" type: SOFTMAX_LOSS bottom: "ip" bottom: "label"
                 top: "loss" }
    """)
    s = SGDSolver(sp, verbose=False)
    assert s.net.layers[0].on_device is False
    assert s.enable_graph() is False
    assert s._use_graph is False and s.net.layers[0].external_staging is False
    s.step(2)
    assert s.iter == 2


def test_image_data_layer_switch_on_equals_switch_off(tmp_path):
    """IMAGE_DATA keeps the decoded image as uint8 on the device path; 5
    images, batch 2, so the list wraps."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(4)
    lines = []
    for i in range(5):
        p = tmp_path / f"im{i}.png"
        Image.fromarray(rng.integers(0, 256, size=(12, 14, 3),
                                     dtype=np.uint8)).save(str(p))
        lines.append(f"{p} {i}")
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    text = f"""
        name: "im"
        layers {{ name: "data" type: IMAGE_DATA top: "data" top: "label"
                 image_data_param {{ source: "{tmp_path / 'list.txt'}"
                                     batch_size: 2 }}
                 transform_param {{ crop_size: 9 mirror: true scale: 0.017
                     mean_value: 104.5 mean_value: 117.25 mean_value: 123.0 }} }}
    """
    runs = {}
    for switch in (False, True):
        pa.init(device="cpu", seed=5, compute_dtype=torch.float32,
                device_transform=switch)
        try:
            net = Net(parse_text("NetParameter", text), phase=TRAIN,
                      verbose=False)
            assert net.layers[0].on_device is switch
            out = []
            for _ in range(4):
                net.forward()
                out.append((net.blobs["data"].data.clone(),
                            net.blobs["label"].data.clone()))
            runs[switch] = out
        finally:
            pa.init(device="cpu", device_transform=False)
    for k in range(4):
        assert runs[True][k][0].shape == (2, 3, 9, 9)
        assert torch.equal(runs[True][k][0], runs[False][k][0]), k
        assert torch.equal(runs[True][k][1], runs[False][k][1]), k
    assert runs[False][2][1].tolist() == [4.0, 0.0]


def test_train_cli_takes_both_flags(files, tmp_path, capsys):
    """--device-transform sets the context switch; --graph reports whether
    enable_graph() took (never on a CPU context) and training goes on."""
    import os
    from poseidon_amd.proto import write_proto_text
    from poseidon_amd.tools.train import main as train_main
    os.environ.pop("RANK", None)
    os.environ.pop("WORLD_SIZE", None)
    net_path = tmp_path / "net.prototxt"
    net_path.write_text('name: "cli"' + data_layer_text(
        files["dir"] / "u8.pdb", 4, "crop_size: 5 mirror: true") + """
        layers { name: "ip" type: INNER_PRODUCT bottom: "data" top: "ip"
                 inner_product_param { num_output: 5
                     weight_filler { type: "gaussian" std: 0.1 } } }
        layers { name: "loss" type: SOFTMAX_LOSS bottom: "ip" bottom: "label"
                 top: "loss" }
    """)
    solver = Message("SolverParameter", net=str(net_path), base_lr=0.01,
                     lr_policy="fixed", max_iter=3, solver_mode="CPU",
                     display=0, snapshot=0, snapshot_after_train=False,
                     random_seed=7)
    sp_path = str(tmp_path / "solver.prototxt")
    write_proto_text(solver, sp_path)
    try:
        train_main(["--solver", sp_path, "--cpu", "--device-transform",
                    "--graph"])
        assert pa.ctx().device_transform is True
        out = capsys.readouterr().out
        assert "hipgraph requested: not capturable, running eager" in out
        assert "hipgraph: false" in out
        assert "optimization done" in out
    finally:
        pa.init(device="cpu", device_transform=False)
    train_main(["--solver", sp_path, "--cpu"])
    assert pa.ctx().device_transform is False
