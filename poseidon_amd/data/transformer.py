"""DataTransformer: mean-subtract, crop, mirror, scale.

Parity: /root/reference/src/caffe/data_transformer.cpp:10-120. Operates on
numpy CHW float32 arrays on the host prefetch path. draw() and device_spec()
split the random draw from the arithmetic, so a data layer can run the
arithmetic on the device (ops.data_transform) over the same draws.
"""

from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from ..proto import Message, read_proto_binary


class DataTransformer:
    def __init__(self, param: Optional[Message], phase: int, rng: np.random.Generator):
        self.phase = phase
        self.rng = rng
        self.scale = 1.0
        self.mirror = False
        self.crop = 0
        self.mean: Optional[np.ndarray] = None
        self.mean_values: Optional[np.ndarray] = None
        if param is not None:
            self.scale = float(param.scale)
            self.mirror = bool(param.mirror)
            self.crop = int(param.crop_size)
            if param.has("mean_file"):
                proto = read_proto_binary(param.mean_file, "BlobProto")
                arr = np.asarray(proto.data, dtype=np.float32)
                self.mean = arr.reshape(proto.channels, proto.height, proto.width)
            elif len(param.mean_value):
                self.mean_values = np.asarray(param.mean_value, dtype=np.float32)

    def draw(self, h: int, w: int) -> Tuple[int, int, int]:
        """(h_off, w_off, flip) of the next h x w datum. Consumes self.rng
        exactly as __call__ does: h_off, then w_off (only when cropping, and
        random only in TRAIN), then the mirror bit (only when mirror and
        TRAIN)."""
        h_off = w_off = 0
        if self.crop:
            cs = self.crop
            if self.phase == 0:  # TRAIN: random crop
                h_off = int(self.rng.integers(0, h - cs + 1))
                w_off = int(self.rng.integers(0, w - cs + 1))
            else:  # TEST: center crop
                h_off = (h - cs) // 2
                w_off = (w - cs) // 2
        flip = bool(self.mirror and self.phase == 0
                    and self.rng.integers(0, 2))
        return h_off, w_off, int(flip)

    def device_spec(self, c: int, h: int, w: int):
        """(mean_mode, mean, scale, crop) for ops.data_transform on c x h x w
        uint8 records; mean is a flat fp32 CPU tensor, or None."""
        import torch
        from ..ops import functional as ops
        if self.mean is not None:
            if self.mean.shape != (c, h, w):
                raise ValueError(
                    f"mean image is {self.mean.shape}, the datum is "
                    f"{(c, h, w)}")
            return (ops.MEAN_IMAGE,
                    torch.from_numpy(np.array(self.mean).reshape(-1)),
                    self.scale, self.crop)
        if self.mean_values is not None:
            mv = self.mean_values
            if mv.size not in (1, c):
                raise ValueError(
                    f"{mv.size} mean_value entries for {c} channels")
            mode = ops.MEAN_SCALAR if mv.size == 1 else ops.MEAN_CHANNEL
            return mode, torch.from_numpy(mv.copy()), self.scale, self.crop
        return ops.MEAN_NONE, None, self.scale, self.crop

    def __call__(self, arr: np.ndarray) -> np.ndarray:
        c, h, w = arr.shape
        h_off, w_off, flip = self.draw(h, w)
        if self.mean is not None:
            arr = arr - self.mean
        elif self.mean_values is not None:
            mv = self.mean_values
            if mv.size == 1:
                arr = arr - mv[0]
            else:
                arr = arr - mv.reshape(c, 1, 1)
        if self.crop:
            cs = self.crop
            arr = arr[:, h_off:h_off + cs, w_off:w_off + cs]
        if flip:
            arr = arr[:, :, ::-1]
        if self.scale != 1.0:
            arr = arr * self.scale
        return np.ascontiguousarray(arr, dtype=np.float32)
