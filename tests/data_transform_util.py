"""Fixtures shared by the device-transform tests (test_data_transform_cpu.py,
test_gpu_data_transform.py): small PDB files of uint8 / float_data records, a
mean file with non-integral values and the DATA-layer net text."""

import numpy as np

from poseidon_amd.data.pdb import PDBWriter, array_to_datum
from poseidon_amd.proto import Message, write_proto_binary


def write_pdb(path, n, c, h, w, seed=5, float_data=False, classes=5):
    """n random c x h x w records with labels i % classes; returns the uint8
    arrays. float_data stores the same values as floats."""
    rng = np.random.default_rng(seed)
    recs = [rng.integers(0, 256, size=(c, h, w), dtype=np.uint8)
            for _ in range(n)]
    with PDBWriter(str(path)) as wtr:
        for i, r in enumerate(recs):
            wtr.put(array_to_datum(r.astype(np.float32) if float_data else r,
                                   i % classes))
    return recs


def write_mean(path, c, h, w, seed=9):
    """A [c,h,w] mean image of non-integral fp32 values around 120."""
    rng = np.random.default_rng(seed)
    mean = (rng.random((c, h, w), dtype=np.float32) * 40 + 100).astype(
        np.float32)
    p = Message("BlobProto", num=1, channels=c, height=h, width=w)
    p.data = mean.ravel()
    write_proto_binary(p, str(path))
    return mean


def data_layer_text(pdb, batch, transform):
    return f"""
    layers {{ name: "data" type: DATA top: "data" top: "label"
             data_param {{ source: "{pdb}" batch_size: {batch} }}
             transform_param {{ {transform} }} }}
    """
