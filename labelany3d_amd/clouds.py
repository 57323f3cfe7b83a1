"""Instance point clouds (include/la3d.h "instance point clouds"): the masked, back-projected pixels of every instance,
``depth_to_points(depth[None], K)[mask]`` (reference src/util.py:52-75, :480-481), for all instances of a batch in one packed array -
the intermediate the fused fit never materialises.  Two C calls on one stream: ``la3d_instance_point_offsets`` (counts and the
offsets of the clouds, scanned on the device) and ``la3d_gather_instance_points`` (the points, in NumPy's row-major order)."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from ._device import _as_dev, _dev, _record, _stream
from .batched import Depth16, _bits_stride, _depth16_block, _depth16_check, _fit_inputs
from .fitcall import depth_rows_for_bits
from .frames import FrameBits, _frames_depth, _on_gpu, _same_table
from .bits import _PackedBits, _mask_bits
from .labels import LabelBits


class InstancePoints(NamedTuple):
    """What ``instance_points`` / ``instance_points_frames`` return, all on the GPU: ``points`` (capacity, 3) float64 or float32 - the
    cloud of instance n is rows ``offsets[n] .. offsets[n+1]`` -, ``offsets`` int64 (B+1,), ``counts`` int32 (B,) - the true pixels of
    every mask (what ``draw_sample_idx`` takes) -, ``pixels`` int32 (capacity,) or None - ``v * frame_width + u`` of every row, so
    ``image.reshape(-1, C)[pixels]`` gathers colours or features -, ``status`` int32 (B,): 0, 1 = the instance's range lies outside
    ``capacity`` (nothing of it is written), 2 = its masks changed between the two stages, 5 = a frames row that breaks the contract.
    ``(ip.points, ip.offsets)`` is what ``fit_points`` takes."""
    points: torch.Tensor
    offsets: torch.Tensor
    counts: torch.Tensor
    pixels: Optional[torch.Tensor]
    status: torch.Tensor


_OUT_DTYPES = (torch.float64, torch.float32)


def _cloud_args(out_dtype, capacity):
    if out_dtype not in _OUT_DTYPES:
        raise ValueError(f"out_dtype must be torch.float64 or torch.float32, not {out_dtype!r}")
    if capacity is not None and (not isinstance(capacity, (int, np.integer)) or isinstance(capacity, bool) or int(capacity) < 0):
        raise ValueError(f"capacity must be None or an int >= 0, not {capacity!r}")


def _run(a: _lib.CloudArgs, B, dev, capacity, out_dtype, pixels, stream, keep, _plan=None, _out=None):
    """Both stages of one call.  ``a``: the block with every input set.  ``_plan`` = (counts, offsets, workspace) of an earlier offsets
    stage: only the gather runs.  ``_out`` = (points, pixels | None, status): buffers to fill instead of fresh ones."""
    with torch.cuda.device(dev):
        s = _stream(stream)
        a.stream = s
        if _plan is None:
            counts = torch.empty(B, dtype=torch.int32, device=dev)
            offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
            ws = torch.empty(max(int(lib.la3d_instance_points_workspace_bytes(B, a.H, a.W)) // 4, 1), dtype=torch.int32, device=dev)
            a.counts, a.offsets, a.workspace = counts.data_ptr(), offsets.data_ptr(), ws.data_ptr()
            check(lib.la3d_instance_point_offsets(C.byref(a)), "la3d_instance_point_offsets")
        else:
            counts, offsets, ws = _plan
            a.counts, a.offsets, a.workspace = counts.data_ptr(), offsets.data_ptr(), ws.data_ptr()
        if _out is not None:
            pts, pix, status = _out
            cap = int(pts.shape[0]) if capacity is None else int(capacity)
        else:
            if capacity is None:
                if stream is not None and stream != torch.cuda.current_stream():
                    stream.synchronize()
                cap = int(offsets[-1].item())   # the ONE synchronisation of the call: the exact size
            else:
                cap = int(capacity)
            pts = torch.empty((cap, 3), dtype=out_dtype, device=dev)
            pix = torch.empty(cap, dtype=torch.int32, device=dev) if pixels else None
            status = torch.empty(B, dtype=torch.int32, device=dev)
        a.points, a.pixels, a.status, a.capacity = pts.data_ptr(), (pix.data_ptr() if pix is not None else None), status.data_ptr(), cap
        a.out_is_f64 = int(pts.dtype == torch.float64)
        check(lib.la3d_gather_instance_points(C.byref(a)), "la3d_gather_instance_points")
    _record(stream, counts, offsets, ws, pts, pix, status, *keep)
    return InstancePoints(pts, offsets, counts, pix, status), ws


def instance_points(depth, masks, K, image_index=None, sample_idx=None, capacity=None, out_dtype=torch.float64, pixels=False, stream=None,
                    device=None, _plan=None, _out=None, _with_plan=False):
    """The point clouds of B instances in one packed array: row ``offsets[n] + r`` of ``points`` is
    ``depth_to_points(depth[img][None], K[img])[masks[n]][r]`` - bit for bit ``unproject(depth, K)[img][masks[n]]`` -, NaN, inf, zero and
    negative depths kept as they come (the cloud before ``estimate_bbox`` drops anything).

    ``masks``: (B,H,W) bool / uint8 (non-zero = True), a ``MaskBits``, or a ``LabelBits`` (its planes and - unless ``image_index`` is
    given - its ``image_index``).  ``depth``: (P,H,W) / (H,W) float32 or a ``Depth16``; for bit planes ``W`` or ``frame_width`` wide
    (padded here as ``fit_instances_bits`` pads it).  ``K``: (3,3) or (P,3,3).  ``image_index``: the plane of every instance (default:
    instance n uses plane n, or the one plane).  ``sample_idx`` (B,500): reference-subsample mode - an instance with more than 500
    pixels gets the 500 rows of the given ranks (``draw_sample_idx(counts)``), every other its whole cloud.
    ``capacity=None`` reads ``offsets[-1]`` back once - the one synchronisation - and allocates exactly; ``capacity=int`` never
    synchronises (an instance that does not fit gets status 1 and is not written), so the call can be captured into a graph.
    ``pixels=True`` adds the flat pixel index of every row.  Returns ``InstancePoints``.
    The ``MaskBits`` that ``pack_rle_bits`` / ``pack_poly_bits`` return is trusted: the packer has just checked and filled the tensor, so
    its layout is not checked a second time here (at one or sixteen instances the call is bound by what this wrapper costs); every
    other ``MaskBits`` - hand-made, from another packer, a ``_replace`` - is checked as ever."""
    _cloud_args(out_dtype, capacity)
    if isinstance(masks, LabelBits):
        image_index = masks.image_index if image_index is None else image_index
        masks = masks.bits
    if isinstance(depth, Depth16):
        _depth16_check(depth)
    a = _lib.CloudArgs(struct_size=C.sizeof(_lib.CloudArgs))
    if isinstance(masks, tuple):
        # (planes straight from pack_rle_bits / pack_poly_bits: that packer has checked the tensor and left its stride)
        stride = getattr(masks, "_stride", None) if isinstance(masks, _PackedBits) else None
        mb = masks if stride is not None else _mask_bits(masks)
        dev = mb.bits.device if device is None else _dev(device)
        if mb.bits.device != dev:
            raise ValueError("the bit planes live on another device")
        B, H, W, fw = int(mb.bits.shape[0]), mb.H, mb.W, mb.frame_width
        if stride is not None and type(depth) is torch.Tensor and depth.dtype == torch.float32 and depth.shape[-1] == W:
            fw_send = 0 if fw == W else fw   # (depth rows as wide as the planes are stored: what depth_rows_for_bits answers)
        else:
            depth, fw_send = depth_rows_for_bits(depth, W, fw, dev)
        a.mask_bits, a.bits_plane_stride, a.frame_width = mb.bits.data_ptr(), stride if stride is not None else _bits_stride(mb.bits, B, H, W), fw_send
        keep, frame = [mb.bits], "the bit-plane frame"
    else:
        if device is None and isinstance(masks, torch.Tensor) and masks.is_cuda:
            device = masks.device
        if np.ndim(masks) != 3:
            raise ValueError("masks must be (B,H,W) bool / uint8, a MaskBits or a LabelBits")
        dev = _dev(device)
        m = _as_dev(masks, torch.uint8, dev)
        B, H, W = (int(x) for x in m.shape)
        a.mask, a.mask_plane_stride = m.data_ptr(), H * W
        keep, frame = [m], "the mask frame"
    d, k, ii, _, si, _ = _fit_inputs(depth, K, image_index, None, sample_idx, B, H, W, dev, frame)
    a.B, a.H, a.W = B, H, W
    if isinstance(d, Depth16):
        blk = _depth16_block(d, H, W)
        a.depth16 = C.pointer(blk)
        keep.append(d.data)
    else:
        a.depth, a.depth_plane_stride = d.data_ptr(), (H * W if d.shape[0] > 1 else 0)
        keep.append(d)
    a.K, a.k_stride = k.data_ptr(), (9 if k.shape[0] > 1 else 0)
    a.image_index = None if ii is None else ii.data_ptr()
    a.sample_idx = None if si is None else si.data_ptr()
    ip, ws = _run(a, B, dev, capacity, out_dtype, pixels, stream, keep + [k, ii, si], _plan, _out)
    return (ip, ws) if _with_plan else ip


def instance_points_frames(frames, bits: FrameBits, K, image_index=None, sample_idx=None, capacity=None, out_dtype=torch.float64,
                           pixels=False, stream=None, _plan=None, _out=None, _with_plan=False):
    """``instance_points`` for instances of images of DIFFERENT sizes: ``frames`` a ``PackedFrames`` / ``PackedFrames16``, ``bits`` the
    ``FrameBits`` laid out by the same frame table (``pack_label_bits_frames`` / ``pack_mask_bits_frames``); ``image_index`` defaults to
    ``bits.image_index``, ``K`` is (3,3) or one matrix per image.  ``pixels`` index each instance's own unpadded image.  An instance whose
    image index, frame row or plane offset breaks the contract gets count 0, status 5 and no rows - decided on the device, never an
    exception.  Other arguments and the result as ``instance_points``."""
    _cloud_args(out_dtype, capacity)
    fdepth, depth = _frames_depth(frames, "instance_points_frames")
    _same_table(frames, bits)
    dev = _on_gpu(fdepth, bits.bits)
    B, P = int(bits.offsets.numel()), int(frames.table.shape[0])
    H, W = max(int(frames.H), 1), max(int(frames.W), 1)
    _, k, ii, _, si, _ = _fit_inputs(None, K, bits.image_index if image_index is None else image_index, None, sample_idx, B, H, W, dev, None,
                                     planes=P, expand_K=False, check_host_index=False)
    a = _lib.CloudArgs(struct_size=C.sizeof(_lib.CloudArgs), B=B, H=H, W=W, P=P)
    if depth.d16 is not None:
        a.depth16 = C.pointer(depth.d16)
    else:
        a.depth = fdepth.data_ptr()
    a.frames, a.mask_bits, a.bits_offsets = frames.table.data_ptr(), bits.bits.data_ptr(), bits.offsets.data_ptr()
    a.K, a.k_stride = k.data_ptr(), (9 if k.shape[0] > 1 else 0)
    a.image_index = ii.data_ptr()
    a.sample_idx = None if si is None else si.data_ptr()
    ip, ws = _run(a, B, dev, capacity, out_dtype, pixels, stream, [fdepth, frames.table, bits.bits, bits.offsets, k, ii, si], _plan, _out)
    return (ip, ws) if _with_plan else ip
