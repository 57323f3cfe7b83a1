"""Morphology on bit planes (include/la3d.h): opening, rectangles and the crop gate, for ``MaskBits`` and - ``*_frames`` - ``FrameBits``;
the depth gate of a ``FrameBits`` (``gate_depth_bits_frames``: the planes of images of different sizes over the depth of their frames)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._device import _as_dev, _int_arg, _ptr, _record, _stream
from ._lib import check, lib
from .batched import _bits_stride, padded_width
from .bits import DepthGateStats, MaskBits, _bits_out, _gate_band, _gate_level, _mask_bits
from .frames import (FrameBits, _bits_buffers, _bounds, _flat_out, _frames_depth, _on_gpu, _same_table, _scaled_table, _tabled, _upscale_arg,
                     frame_bits_offsets)


def _open_scalars(who: str, k, upscale) -> None:   # the k and upscale of an opening, of either form
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 31 or int(k) % 2 == 0:
        raise ValueError(f"{who}: k must be an odd int in 1 .. 31, not {k!r}")
    _upscale_arg(who, upscale)


def _gate_scalars(who: str, min_area, crop_size) -> None:   # the gate of select_crops, of either form
    _int_arg(who, "min_area", min_area, 0)
    if isinstance(crop_size, bool) or not isinstance(crop_size, (int, np.integer)) or int(crop_size) <= 0:
        raise ValueError(f"{who}: crop_size must be an int > 0, not {crop_size!r}")


def _open_args(who: str, bits, k, upscale) -> MaskBits:
    if not isinstance(bits, MaskBits):
        raise ValueError(f"{who}: bits must be a MaskBits (pack_mask_bits, pack_rle_bits, pack_poly_bits, pack_crop_bits, ...)")
    _open_scalars(who, k, upscale)
    mb = _mask_bits(bits)
    if mb.H <= 0:
        raise ValueError(f"{who}: the planes state an empty frame {(mb.H, mb.W)}")
    return mb


def _open_run(who: str, mb: MaskBits, k: int, s: int, W_out: int, out, want_stats: bool, stream):
    """One ``la3d_open_bits`` call on checked arguments -> (out, stats); ``out`` None: statistics only."""
    B, dev = int(mb.bits.shape[0]), mb.bits.device
    out_stride = 0 if out is None else _bits_stride(out, B, s * mb.H, W_out)
    with torch.cuda.device(dev):
        stats = ws = None
        if want_stats:
            stats = torch.empty((B, 5), dtype=torch.int32, device=dev)
            ws = torch.empty(max(int(lib.la3d_open_bits_workspace_bytes(B, mb.H, s)) // 4, 1), dtype=torch.int32, device=dev)
        if B:   # (an empty batch has no planes to point at)
            check(lib.la3d_open_bits(_ptr(mb.bits), _bits_stride(mb.bits, B, mb.H, mb.W), B, mb.H, mb.W, mb.frame_width, k, s,
                                     _ptr(out), out_stride, W_out, _ptr(stats), _ptr(ws), _stream(stream)), "la3d_open_bits")
    _record(stream, mb.bits, out, stats, ws)
    return out, stats


def open_bits(bits: MaskBits, k: int = 7, upscale: int = 1, frame_pad: bool = True, stream=None, out=None, return_stats: bool = False):
    """Binary opening of bit planes on the GPU (C-ABI ``la3d_open_bits``): ``scipy.ndimage.binary_opening(U, np.ones((k, k)))`` of the
    nearest-neighbour upscale ``U[v, u] = M[v // s, u // s]`` of every plane, ``s = upscale`` - the crop stage's mask step (reference
    src/batch_scripts/get_crops_enhanced.py:68-88: x4, k = 7); at ``upscale=1`` it strips speckle and hairlines from network masks
    before a fit.  ``k``: odd, 1 .. 31 (1 = identity); ``upscale``: 1, 2 or 4.  Returns ``MaskBits`` of ``s*H`` rows and ``s*frame_width``
    image columns, stored ``padded_width(s*frame_width)`` wide with ``frame_pad`` (else unpadded) - or ``(MaskBits, stats)`` with
    ``return_stats``: ``stats`` int32 (B, 5) on the device, ``area, x, y, w, h`` of each opened plane (``cv2.boundingRect``'s
    convention; zeros for an empty plane).  ``out``: an int32 (B, >= words) device tensor to fill; it must not overlap the input (the
    call cannot work in place).  No host synchronisation; capturable."""
    who = "open_bits"
    mb = _open_args(who, bits, k, upscale)
    k, s = int(k), int(upscale)
    B, dev = int(mb.bits.shape[0]), mb.bits.device
    fw = s * mb.frame_width
    W_out = padded_width(fw) if frame_pad else fw
    if out is not None and isinstance(out, torch.Tensor) and out.device != dev:
        raise ValueError(f"{who}: out lives on another device")
    o = _bits_out(out, B, s * mb.H, W_out, dev)
    o, stats = _open_run(who, mb, k, s, W_out, o, bool(return_stats), stream)
    res = MaskBits(o, s * mb.H, W_out, fw)
    return (res, stats) if return_stats else res


def bits_rects(bits: MaskBits, stream=None) -> torch.Tensor:
    """``MaskBits`` -> int32 (B, 5) on the device: ``area, x, y, w, h`` of every plane - the statistics-only call of ``la3d_open_bits``
    with ``k = 1, upscale = 1`` (nothing but the planes is read, no plane is written)."""
    mb = _open_args("bits_rects", bits, 1, 1)
    return _open_run("bits_rects", mb, 1, 1, mb.frame_width, None, True, stream)[1]


def crop_params(stats, crop_size: int = 512, upscale: int = 4, ratio: float = 0.7) -> np.ndarray:
    """The crop parameters of the reference's crop stage from the rectangles of opened planes: ``stats`` (B, 5) ``area, x, y, w, h``
    (``open_bits(..., return_stats=True)``, ``bits_rects``; a (B, 4) array is taken as ``x, y, w, h``) -> float64 (B, 3) rows
    ``(offset_x, offset_y, scale_factor)``, what ``crop_placement`` / ``pack_crop_bits`` take.  Host arithmetic on Python numbers,
    exactly the reference's (``crop_object``, src/util.py:142-157, then src/batch_scripts/get_crops_enhanced.py:98):
    ``side = int(max(w, h) / ratio)``, ``ox = x + (w - side) / 2``, ``oy = y + (h - side) / 2``, ``sf = crop_size / side``; the row is
    ``[ox / upscale, oy / upscale, sf * upscale]`` - the rectangle is measured on the upscaled image, the parameters speak of the
    original one.  Rows with ``w == 0`` (an empty plane) are NaN."""
    a = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    if a.ndim != 2 or a.shape[1] not in (4, 5):
        raise ValueError(f"crop_params: stats must be (B, 5) area, x, y, w, h or (B, 4) x, y, w, h, got {a.shape}")
    if not (crop_size > 0 and upscale > 0 and ratio > 0):
        raise ValueError("crop_params: crop_size, upscale and ratio must be positive")
    out = np.full((a.shape[0], 3), np.nan, np.float64)
    for n, row in enumerate(a[:, -4:].tolist()):
        x, y, w, h = (int(v) for v in row)
        if w <= 0 or h <= 0:
            continue
        side = int(max(w, h) / ratio)
        ox, oy, sf = x + (w - side) / 2, y + (h - side) / 2, crop_size / side
        out[n] = [ox / upscale, oy / upscale, sf * upscale]
    return out


def select_crops(bits: MaskBits, min_area: int = 6400, k: int = 7, upscale: int = 4, crop_size: int = 512, stream=None):
    """The instance selection of the reference's crop stage (src/batch_scripts/get_crops_enhanced.py:68-99) for a batch of planes:
    ``open_bits(bits, k, upscale)``, then ``keep = area >= min_area`` and ``crop_params`` of the rectangles -> ``(keep, params, stats,
    opened)``: ``keep`` bool (B,) and ``params`` float64 (B, 3) NumPy arrays (NaN rows for empty planes), ``stats`` int32 (B, 5) on the
    device, ``opened`` the ``MaskBits`` of the opened, upscaled planes.  The defaults are the reference's gate (x4, 7 x 7, 6400
    surviving pixels, 512-pixel crops); one device-to-host copy (the statistics).  The reference walks the instances LAST TO FIRST and
    appends the boxes it keeps to ``bboxes.json`` in that order: rows here stay in the caller's order, and the order of
    ``bboxes.json`` is the caller's business."""
    _gate_scalars("select_crops", min_area, crop_size)
    opened, stats = open_bits(bits, k=k, upscale=upscale, frame_pad=True, stream=stream, return_stats=True)
    if stream is not None and stream != torch.cuda.current_stream():
        stream.synchronize()
    host = stats.cpu().numpy()
    return host[:, 0] >= int(min_area), crop_params(host, crop_size=int(crop_size), upscale=int(upscale)), stats, opened


def _open_frames_run(frames, bits: FrameBits, k: int, s: int, out, offs, stream):
    """One ``la3d_open_bits_frames`` call on checked arguments -> stats int32 (B, 5); ``out`` None: statistics only."""
    dev = bits.bits.device
    B, P = int(bits.offsets.numel()), int(frames.table.shape[0])
    with torch.cuda.device(dev):
        ii = _as_dev(bits.image_index, torch.int32, dev)
        stats = torch.empty((B, 5), dtype=torch.int32, device=dev)
        ws = torch.empty(max(int(lib.la3d_open_bits_frames_workspace_bytes(B, max(int(frames.H), 1), s)) // 4, 1), dtype=torch.int32, device=dev)
        if B:   # (an empty batch has no planes to point at)
            check(lib.la3d_open_bits_frames(_ptr(bits.bits), int(bits.bits.numel()), _ptr(bits.offsets), _ptr(frames.table) if P else None, P,
                                            max(int(frames.H), 1), max(int(frames.W), 1), _ptr(ii), B, k, s, _ptr(out),
                                            0 if out is None else int(out.numel()), _ptr(offs), _ptr(stats), _ptr(ws), _stream(stream)),
                  "la3d_open_bits_frames")
    _record(stream, bits.bits, bits.offsets, frames.table, ii, out, offs, stats, ws)
    return stats


def open_bits_frames(frames, bits: FrameBits, k: int = 7, upscale: int = 1, image_index=None, stream=None, out=None,
                     return_stats: bool = False):
    """``open_bits`` for the planes of images of DIFFERENT sizes in one call (C-ABI ``la3d_open_bits_frames``): the opening by
    ``np.ones((k, k))`` of the nearest x ``upscale`` upscale of every plane of ``bits``, each over its OWN image.  ``frames``: a
    ``PackedFrames`` / ``PackedFrames16`` / ``PackedLabels`` / ``PackedMasks`` / ``FrameGrid`` whose frame table the planes were
    laid out for (another table: ValueError before any device work); ``k``: odd, 1 .. 31; ``upscale``: 1, 2 or 4 - ONE of each per
    call.  The plane of an image of size (h, w) comes back as the plane of an image of size (s*h, s*w): ``s*h`` rows,
    ``padded_width(s*w)`` wide, the bits of the padding columns zero.  ``image_index``: None, or a HOST copy of the indices the planes
    were packed with - the opened planes are then laid out compactly (``frame_bits_offsets`` on the scaled table; the offsets go up in
    one copy); None never synchronises and lays the planes a uniform stride apart, the words of the scaled bounds' frame rounded up to
    4 (at x4 sixteen times the largest source plane per row, whatever the row's own size).  ``out``: a flat, 16-byte aligned int32
    device tensor of at least that many words to fill; it must not overlap ``bits.bits`` (the call cannot work in place).
    Returns ``FrameBits`` - ``image_index`` the input's, ``area`` the opened area, ``table`` / ``H`` / ``W`` the input's at
    ``upscale=1`` (the result goes straight into ``fit_instances_frames_bits``, ``instance_points_frames`` and
    ``rle_encode_bits_frames`` with the same ``frames``), else those of ``scaled_frames(frames, upscale)`` - or, with
    ``return_stats``, ``(FrameBits, stats)``: int32 (B, 5) on the device, ``area, x, y, w, h`` of each opened plane.  A row whose image
    index, frame row or plane offset breaks the contract, or whose plane does not end inside its buffer, writes no word and gets
    ``-1, 0, 0, 0, 0`` (``area`` 0 in the ``FrameBits``) - decided on the device, never an exception.  No host synchronisation;
    capturable."""
    who = "open_bits_frames"
    _tabled(who, frames, bits)
    _open_scalars(who, k, upscale)
    k, s = int(k), int(upscale)
    B, P = int(bits.offsets.numel()), len(frames.table_host)
    table = frames.table_host if s == 1 else _scaled_table(frames.table_host, s)
    H_s, W_s = _bounds(table)
    offs_h = None
    if image_index is not None:
        if isinstance(image_index, torch.Tensor) and image_index.is_cuda:
            raise ValueError(f"{who}: image_index must be a host copy of the planes' image indices (None: the uniform-stride layout)")
        ii = np.asarray(image_index.numpy() if isinstance(image_index, torch.Tensor) else image_index).reshape(-1)
        if len(ii) != B or (B and not np.issubdtype(ii.dtype, np.integer)):
            raise ValueError(f"{who}: image_index must hold one integer image index per plane ({B}), got {len(ii)} of {ii.dtype}")
        if B and (int(ii.min()) < 0 or int(ii.max()) >= P):
            raise ValueError(f"{who}: image_index must lie in [0, {P})")
        offs_h, total = frame_bits_offsets(table, ii)
    else:
        stride = (H_s * W_s // 32 + 3) // 4 * 4
        total = B * stride
    _flat_out(who, out, None, bits.bits)   # (the in-place refusal alone: the buffer itself is judged on its device, below)
    dev = _on_gpu(frames.table, bits.bits)
    with torch.cuda.device(dev):
        o, _ = _bits_buffers(out, total, 0, dev)
        offs = _as_dev(offs_h, torch.int64, dev) if offs_h is not None else torch.arange(B, dtype=torch.int64, device=dev) * stride
        stats = _open_frames_run(frames, bits, k, s, o, offs, stream)
        area = stats[:, 0].clamp(min=0).contiguous()
    _record(stream, area)
    res = FrameBits(o, offs, bits.image_index, area, table, H_s, W_s)
    return (res, stats) if return_stats else res


def bits_rects_frames(frames, bits: FrameBits, stream=None) -> torch.Tensor:
    """``FrameBits`` -> int32 (B, 5) on the device: ``area, x, y, w, h`` of every plane over its own image - the statistics-only call
    of ``la3d_open_bits_frames`` with ``k = 1, upscale = 1`` (no plane is written); ``-1, 0, 0, 0, 0`` for a row the device refuses.
    ``frames`` as in ``open_bits_frames``."""
    _tabled("bits_rects_frames", frames, bits)
    _on_gpu(frames.table, bits.bits)
    return _open_frames_run(frames, bits, 1, 1, None, None, stream)


def select_crops_frames(frames, bits: FrameBits, min_area: int = 6400, k: int = 7, upscale: int = 4, crop_size: int = 512, image_index=None,
                        stream=None):
    """``select_crops`` for the planes of images of DIFFERENT sizes - the instance selection of the reference's crop stage
    (src/batch_scripts/get_crops_enhanced.py:68-99) for a whole shard in one call: ``open_bits_frames(frames, bits, k, upscale,
    image_index)``, then ``keep = area >= min_area`` and ``crop_params`` of the rectangles -> ``(keep, params, stats, opened)``:
    ``keep`` bool (B,) and ``params`` float64 (B, 3) NumPy arrays - false and NaN for empty planes and for rows the device refuses
    (``stats`` row ``-1, 0, 0, 0, 0``) -, ``stats`` int32 (B, 5) on the device, ``opened`` the ``FrameBits`` of the opened, upscaled
    planes.  ``params`` speak of the ORIGINAL frames: they are what ``pack_crop_bits_frames(frames, crops, params, image_index)`` takes.
    The defaults are the reference's gate (x4, 7 x 7, 6400 surviving pixels, 512-pixel crops); one device-to-host copy (the
    statistics).  The reference walks the instances LAST TO FIRST and appends the boxes it keeps to ``bboxes.json`` in that order: rows
    here stay in the caller's order, and the order of ``bboxes.json`` is the caller's business."""
    _gate_scalars("select_crops_frames", min_area, crop_size)
    opened, stats = open_bits_frames(frames, bits, k=k, upscale=upscale, image_index=image_index, stream=stream, return_stats=True)
    if stream is not None and stream != torch.cuda.current_stream():
        stream.synchronize()
    host = stats.cpu().numpy()
    return host[:, 0] >= int(min_area), crop_params(np.maximum(host, 0), crop_size=int(crop_size), upscale=int(upscale)), stats, opened


# ---- the depth gate of a FrameBits (include/la3d.h "depth gate on bit planes": la3d_depth_gate_bits_frames) ---------------------------
def _gate_frames_run(who: str, frames, bits, k, min_band, near, far, stream, out, want_plane: bool, want_stats: bool):
    """The checks of ``gate_depth_bits_frames`` / ``depth_gate_stats_frames`` and one ``la3d_depth_gate_bits_frames`` call ->
    (FrameBits or None, stats or None)."""
    flat, depth = _frames_depth(frames, who)   # (a PackedFrames / PackedFrames16: the call reads depth)
    _same_table(frames, bits)
    k, min_band = _gate_band(who, "k", k), _gate_band(who, "min_band", min_band)
    near, far = _gate_level(who, "near", near, float("-inf")), _gate_level(who, "far", far, float("inf"))
    H, W = max(int(frames.H), 1), max(int(frames.W), 1)
    if H * W > _lib.DEPTH_GATE_MAX_PIXELS:
        raise ValueError(f"{who}: bounds of {(H, W)} have more than {_lib.DEPTH_GATE_MAX_PIXELS} stored pixels")
    total = int(bits.bits.numel())
    in_place = isinstance(out, torch.Tensor) and out.dtype == torch.int32 and out.dim() == 1 and out.numel() == total and \
        out.data_ptr() == bits.bits.data_ptr()
    if want_plane and not in_place:
        _flat_out(who, out, total, bits.bits)
    dev = _on_gpu(flat, bits.bits)
    if frames.table.device != dev or (out is not None and out.device != dev):
        raise ValueError(f"{who}: the frame table or out lives on another device")
    B, P = int(bits.offsets.numel()), int(frames.table.shape[0])
    with torch.cuda.device(dev):
        o = None if not want_plane else torch.empty(max(total, 4), dtype=torch.int32, device=dev) if out is None else out
        ii = _as_dev(bits.image_index, torch.int32, dev)
        counts = torch.empty((B, 3), dtype=torch.int32, device=dev)   # (always: the area of the result comes from it)
        levels = torch.empty((B, 3), dtype=torch.float32, device=dev) if want_stats else None
        if B:   # (an empty batch has no planes to point at)
            a = _lib.DepthGateFramesArgs(struct_size=C.sizeof(_lib.DepthGateFramesArgs), B=B, P=P, H=H, W=W, k=k, min_band=min_band, near=near,
                                         far=far, depth=flat.data_ptr() if depth.d16 is None else None,
                                         depth16=None if depth.d16 is None else C.pointer(depth.d16), depth_elems=int(flat.numel()),
                                         frames=frames.table.data_ptr() if P else None, image_index=ii.data_ptr(),
                                         bits=bits.bits.data_ptr(), bits_words=total, bits_offsets=bits.offsets.data_ptr(),
                                         out_bits=None if o is None else o.data_ptr(), out_words=0 if o is None else int(o.numel()),
                                         out_offsets=None if o is None else bits.offsets.data_ptr(),
                                         counts=counts.data_ptr(), levels=None if levels is None else levels.data_ptr(), stream=_stream(stream))
            check(lib.la3d_depth_gate_bits_frames(C.byref(a)), "la3d_depth_gate_bits_frames")
        res = None
        if want_plane:
            area = torch.empty(B, dtype=torch.int32, device=dev)
            with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):   # behind the kernel, on ITS stream
                torch.clamp(counts[:, 2], min=0, out=area)
            res = FrameBits(o, bits.offsets, bits.image_index, area, bits.table, bits.H, bits.W)
            _record(stream, area)
    _record(stream, flat, frames.table, ii, bits.bits, bits.offsets, o, counts, levels)
    return res, (DepthGateStats(counts, levels) if want_stats else None)


def gate_depth_bits_frames(frames, bits: FrameBits, k: float = 4.5, min_band: float = 0.0, near=None, far=None, stream=None, out=None,
                           return_stats: bool = False):
    """``gate_depth_bits`` for the planes of images of DIFFERENT sizes in one call, over depth as it is stored (C-ABI
    ``la3d_depth_gate_bits_frames``): every plane of ``bits`` loses its depth outliers over its OWN image's depth plane before
    ``fit_instances_frames_bits`` takes every set pixel - the rule, ``k``, ``min_band``, ``near`` and ``far`` of ``gate_depth_bits``,
    ONE of each per call.  ``frames``: the ``PackedFrames`` (float32) or ``PackedFrames16`` (float16 / uint16, gated where it lies: the
    value of a stored word is the fit's - float16 exact, uint16 one rounded ``float32(x) * scale``, a stored 0 a hole with
    ``zero_is_hole`` - and the result is, word for word, the float32 call's on the up-converted planes) whose frame table the planes
    were laid out for (another table, or a ``frames`` without depth: ValueError before any device work).  Bounds of more than 857728
    stored pixels are refused.  ``out``: None (a fresh tensor), a flat, 16-byte aligned int32 device tensor of at least
    ``bits.bits.numel()`` words to fill, or ``bits.bits`` itself (in place); any other overlap with the input is refused.  Returns
    ``FrameBits(out, bits.offsets, bits.image_index, area, bits.table, bits.H, bits.W)`` - the planes lie where the input's lie in
    their buffer, the offsets tensor is shared, ``area`` is the kept area -, which goes straight into ``fit_instances_frames_bits`` and
    every other frames consumer with the same ``frames``; or ``(FrameBits, DepthGateStats)`` with ``return_stats``.  A row whose
    image index, frame row or plane offset breaks the contract, or whose plane or depth plane does not end inside its buffer, writes no
    word and gets ``counts = -2, 0, 0`` and NaN levels (``area`` 0 in the ``FrameBits``) - decided on the device, never an exception.
    One kernel, no host synchronisation and no host copy of the image indices; capturable."""
    res, stats = _gate_frames_run("gate_depth_bits_frames", frames, bits, k, min_band, near, far, stream, out, True, bool(return_stats))
    return (res, stats) if return_stats else res


def depth_gate_stats_frames(frames, bits: FrameBits, k: float = 4.5, min_band: float = 0.0, near=None, far=None, stream=None) -> DepthGateStats:
    """The ``DepthGateStats`` of ``gate_depth_bits_frames`` without its planes (``out_bits = NULL``: no plane is written)."""
    return _gate_frames_run("depth_gate_stats_frames", frames, bits, k, min_band, near, far, stream, None, False, True)[1]
