"""16-bit depth planes (include/la3d.h "16-bit depth planes"): float32 depth -> ``Depth16`` (float16 / uint16) and back, on the device
(``pack_depth16`` / ``unpack_depth16``).  ``Depth16`` itself and its checks live in ``batched``; ``masks`` re-exports the public names."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from ._device import _dev, _plane_source, _ptr, _record, _stream
from .batched import Depth16, _depth16_block, _depth16_check, padded_width

_D16_DTYPES = {"f16": (torch.float16, _lib.DTYPE_F16), "u16": (torch.uint16, _lib.DTYPE_U16)}


def pack_depth16(depth, dtype: str = "f16", scale: float = 0.001, frame_pad: bool = False, device=None, stream=None, out=None) -> Depth16:
    """(P,H,W) or (H,W) float32 depth -> ``Depth16`` on the GPU (C-ABI ``la3d_pack_depth16``).  ``dtype`` "f16": IEEE half, round to
    nearest even, overflow to inf, subnormals kept (``astype(np.float16)``); "u16": ``rint(d / scale)`` in float32 - NaN, +-inf and
    d <= 0 give 0 (a hole: the result has ``zero_is_hole=True``), more than 65535 units give 65535 -, ``scale`` metres per unit
    (0.001: millimetres; ignored for "f16").  ``frame_pad``: rows of a width that is not a multiple of 32 are padded with zeros to
    ``padded_width(W)`` (``frame_width`` of the result keeps W), which is what the tiled forms of the fit want with run-length /
    polygon / bit-plane masks.  A device tensor with dense planes is read in place.  ``out``: a float16 / uint16 device tensor
    (P,H,W_out) to fill, whose planes may lie further apart (only the words of each plane are written)."""
    if dtype not in _D16_DTYPES:
        raise ValueError(f"unknown dtype: {dtype!r}. Use 'f16' or 'u16'")
    tdt, code = _D16_DTYPES[dtype]
    if dtype == "u16" and not (np.isfinite(np.float32(scale)) and np.float32(scale) > 0):
        raise ValueError(f"scale must be finite and > 0 (as float32), not {scale!r}")
    if device is None and isinstance(depth, torch.Tensor) and depth.is_cuda:
        device = depth.device
    dev = _dev(device)
    two_d = np.ndim(depth) == 2
    x, ps = _plane_source(depth[None] if two_d else depth, dev, (torch.float32,))
    P, H, W = x.shape
    W_out = padded_width(W) if frame_pad else W
    if out is None:
        o = torch.empty((P, H, W_out), dtype=tdt, device=dev)
    else:
        o = out[None] if out.dim() == 2 else out
        if not (o.is_cuda and o.dtype == tdt and tuple(o.shape) == (P, H, W_out)):
            raise ValueError(f"out must be a {tdt} device tensor of shape {(P, H, W_out)}")
        _depth16_block(Depth16(o), H, W_out)   # (dense rows, planes >= H*W_out elements apart)
    with torch.cuda.device(dev):
        check(lib.la3d_pack_depth16(_ptr(x), ps, P, H, W, W_out, code, float(scale), _ptr(o), int(o.stride(0)) if P > 1 else H * W_out,
                                    _stream(stream)), "la3d_pack_depth16")
    _record(stream, x, o)
    return Depth16(o[0] if two_d else o, float(scale) if dtype == "u16" else 1.0, True, W if W_out != W else 0)


def unpack_depth16(d16: Depth16, stream=None) -> torch.Tensor:
    """``Depth16`` -> the float32 planes the fit sees, (P,H,W) or (H,W) like ``d16.data`` (the first ``frame_width`` columns when
    the rows are padded), on the GPU (C-ABI ``la3d_unpack_depth16``): float32(x) for float16 planes, float32(x) * float32(scale)
    for uint16 planes, a stored 0 as NaN with ``zero_is_hole``."""
    if not isinstance(d16, Depth16):
        raise ValueError("unpack_depth16 takes a Depth16")
    _depth16_check(d16)
    t = d16.data if d16.data.dim() == 3 else d16.data[None]
    P, H, W_in = t.shape
    blk = _depth16_block(d16._replace(data=t), H, W_in)
    W = int(d16.frame_width) or W_in
    out = torch.empty((P, H, W), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        check(lib.la3d_unpack_depth16(C.byref(blk), P, H, W_in, W, _ptr(out), _stream(stream)), "la3d_unpack_depth16")
    _record(stream, t, out)
    return out if d16.data.dim() == 3 else out[0]
