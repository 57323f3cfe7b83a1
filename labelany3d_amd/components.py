"""Connected components on bit planes (include/la3d.h "connected components on bit planes"): keep the largest part of every mask, or
drop its islands under an area, on the GPU - ``scipy.ndimage.label`` + ``np.bincount`` for a batch of ``MaskBits`` without the unpack /
device-to-host copy / pack round trip.  ``components_bits`` is the general form; ``largest_component_bits`` and ``drop_islands_bits``
are its two thin forms, ``components_stats`` the statistics-only call.  ``components_bits_frames``, ``largest_component_bits_frames``,
``drop_islands_bits_frames`` and ``components_stats_frames`` are the same four for the ``FrameBits`` of images of different sizes
(C-ABI ``la3d_components_bits_frames``): one call for a whole shard."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._device import _as_dev, _int_arg, _record, _stream
from ._lib import check, lib
from .batched import _bits_stride
from .bits import MaskBits, _bits_out, _mask_bits
from .frames import FrameBits, _flat_out, _on_gpu, _tabled


def _components_scalars(who: str, min_area, largest, connectivity, max_components, max_runs) -> None:
    _int_arg(who, "min_area", min_area, 0)
    if not isinstance(largest, (bool, np.bool_)) and not (isinstance(largest, (int, np.integer)) and int(largest) in (0, 1)):
        raise ValueError(f"{who}: largest must be a bool, not {largest!r}")
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or int(connectivity) not in (4, 8):
        raise ValueError(f"{who}: connectivity must be 4 or 8, not {connectivity!r}")
    _int_arg(who, "max_components", max_components, 0)
    _int_arg(who, "max_runs", max_runs, 1, _lib.COMPONENTS_MAX_RUNS)


def _components_args(who: str, bits, min_area, largest, connectivity, max_components, max_runs) -> MaskBits:
    if not isinstance(bits, MaskBits):
        raise ValueError(f"{who}: bits must be a MaskBits (pack_mask_bits, pack_rle_bits, pack_poly_bits, pack_crop_bits, ...)")
    _components_scalars(who, min_area, largest, connectivity, max_components, max_runs)
    H, W = int(bits.H), int(bits.W)
    if H <= 0 or W <= 0:
        raise ValueError(f"{who}: the planes state an empty frame {(H, W)}")
    if H * W > 1048576:
        raise ValueError(f"{who}: a frame of {(H, W)} has more than 1048576 pixels")
    return _mask_bits(bits)


def _components_run(who: str, mb: MaskBits, min_area, largest, connectivity, max_components, max_runs, out, want_stats, stream):
    """One ``la3d_components_bits`` call on checked arguments -> (out, stats, components); ``out`` None: no plane is written."""
    B, dev = int(mb.bits.shape[0]), mb.bits.device
    maxc = int(max_components)
    with torch.cuda.device(dev):
        stats = torch.empty((B, 8), dtype=torch.int32, device=dev) if want_stats else None
        comps = torch.empty((B, maxc, 5), dtype=torch.int32, device=dev) if maxc else None
        ws = torch.empty(max(int(lib.la3d_components_workspace_bytes(B, mb.H, int(max_runs))) // 4, 1), dtype=torch.int32, device=dev)
        if B:   # (an empty batch has no planes to point at)
            a = _lib.ComponentsArgs(struct_size=C.sizeof(_lib.ComponentsArgs), B=B, H=mb.H, W=mb.W,
                                    frame_width=0 if mb.frame_width == mb.W else mb.frame_width, connectivity=int(connectivity),
                                    min_area=int(min_area), largest=int(bool(largest)), max_runs=int(max_runs), max_components=maxc,
                                    mask_bits=mb.bits.data_ptr(), bits_plane_stride=_bits_stride(mb.bits, B, mb.H, mb.W),
                                    out_bits=None if out is None else out.data_ptr(),
                                    out_plane_stride=0 if out is None else _bits_stride(out, B, mb.H, mb.W),
                                    stats=None if stats is None else stats.data_ptr(), components=None if comps is None else comps.data_ptr(),
                                    workspace=ws.data_ptr(), stream=_stream(stream))
            check(lib.la3d_components_bits(C.byref(a)), "la3d_components_bits")
    _record(stream, mb.bits, out, stats, comps, ws)
    return out, stats, comps


def components_bits(bits: MaskBits, min_area: int = 0, largest: bool = False, connectivity: int = 8, max_components: int = 0,
                    max_runs: int = 16384, stream=None, out=None, return_stats: bool = False):
    """Connected components of bit planes on the GPU (C-ABI ``la3d_components_bits``): per plane ``labels, n = scipy.ndimage.label(M,
    structure)`` - ``connectivity=8``: ``np.ones((3, 3))``, ``connectivity=4``: the cross -, the components of ``area >= min_area`` are
    the candidates, ``largest=False`` keeps every candidate, ``largest=True`` only the one of greatest area (ties: the lowest label,
    i.e. the component whose first pixel comes first in raster order).  Returns the ``MaskBits`` of the kept components, in the input's
    geometry - or ``(MaskBits, stats)`` with ``return_stats``, or ``(MaskBits, stats, components)`` when ``max_components > 0``:
    ``stats`` int32 (B, 8) on the device, ``n_components, n_kept, area_in, area_out, x, y, w, h`` (the rectangle of the output,
    ``cv2.boundingRect``'s convention, zeros when empty); ``components`` int32 (B, max_components, 5), ``area, x, y, w, h`` of label
    ``j + 1`` in row ``j`` (zeros beyond ``n_components``).  ``max_runs``: the horizontal runs one plane may have (16384 covers a noisy
    640 x 480 mask); a plane with more gets ``stats = -1, runs, 0, ...``, an all-zero plane and zero table rows - call again with
    ``max_runs >= runs``.  ``out``: an int32 (B, >= words) device tensor to fill; it must not overlap the input.  No host
    synchronisation; capturable."""
    who = "components_bits"
    mb = _components_args(who, bits, min_area, largest, connectivity, max_components, max_runs)
    B, dev = int(mb.bits.shape[0]), mb.bits.device
    if out is not None and isinstance(out, torch.Tensor) and out.device != dev:
        raise ValueError(f"{who}: out lives on another device")
    o = _bits_out(out, B, mb.H, mb.W, dev)
    want = bool(return_stats) or int(max_components) > 0
    o, stats, comps = _components_run(who, mb, min_area, largest, connectivity, max_components, max_runs, o, want, stream)
    res = MaskBits(o, mb.H, mb.W, mb.frame_width)
    if int(max_components) > 0:
        return res, stats, comps
    return (res, stats) if return_stats else res


def components_stats(bits: MaskBits, min_area: int = 0, largest: bool = False, connectivity: int = 8, max_components: int = 0,
                     max_runs: int = 16384, stream=None):
    """The statistics of ``components_bits`` without its planes (``out_bits = NULL``: nothing but the planes is read): ``stats`` int32
    (B, 8), or ``(stats, components)`` when ``max_components > 0``."""
    who = "components_stats"
    mb = _components_args(who, bits, min_area, largest, connectivity, max_components, max_runs)
    _, stats, comps = _components_run(who, mb, min_area, largest, connectivity, max_components, max_runs, None, True, stream)
    return (stats, comps) if int(max_components) > 0 else stats


def largest_component_bits(bits: MaskBits, connectivity: int = 8, min_area: int = 0, max_runs: int = 16384, stream=None, out=None,
                           return_stats: bool = False):
    """The largest connected component of every plane (``components_bits(largest=True)``): what makes one object of an occluded
    instance's polygon parts or of a network mask with far islands before ``fit_instances_bits`` takes every set pixel."""
    return components_bits(bits, min_area=min_area, largest=True, connectivity=connectivity, max_runs=max_runs, stream=stream, out=out,
                           return_stats=return_stats)


def drop_islands_bits(bits: MaskBits, min_area: int, connectivity: int = 8, max_runs: int = 16384, stream=None, out=None,
                      return_stats: bool = False):
    """Every plane without its components of fewer than ``min_area`` pixels (``components_bits(min_area=...)``); ``min_area=0`` is the
    identity on the image columns.  Unlike ``open_bits`` it removes by component, not by shape: thin true structure stays."""
    return components_bits(bits, min_area=min_area, largest=False, connectivity=connectivity, max_runs=max_runs, stream=stream, out=out,
                           return_stats=return_stats)


# ---- the planes of images of different sizes (include/la3d.h "connected components on bit planes", la3d_components_bits_frames) ------
def _components_frames_check(who: str, frames, bits, min_area, largest, connectivity, max_components, max_runs) -> None:
    _tabled(who, frames, bits)
    _components_scalars(who, min_area, largest, connectivity, max_components, max_runs)
    H, W = int(frames.H), int(frames.W)
    if H * ((W + 31) // 32 * 32) > 1048576:
        raise ValueError(f"{who}: the bounds {(H, W)} of the frame table have more than 1048576 pixels")


def _components_frames_run(frames, bits: FrameBits, min_area, largest, connectivity, max_components, max_runs, out, want_stats, stream):
    """One ``la3d_components_bits_frames`` call on checked arguments -> (stats, components); ``out`` None: no plane is written."""
    dev = bits.bits.device
    B, P, maxc = int(bits.offsets.numel()), int(frames.table.shape[0]), int(max_components)
    H, W = max(int(frames.H), 1), max(int(frames.W), 1)
    with torch.cuda.device(dev):
        ii = _as_dev(bits.image_index, torch.int32, dev)
        stats = torch.empty((B, 8), dtype=torch.int32, device=dev) if want_stats else None
        comps = torch.empty((B, maxc, 5), dtype=torch.int32, device=dev) if maxc else None
        ws = torch.empty(max(int(lib.la3d_components_workspace_bytes(B, H, int(max_runs))) // 4, 1), dtype=torch.int32, device=dev)
        if B:   # (an empty batch has no planes to point at)
            a = _lib.ComponentsFramesArgs(struct_size=C.sizeof(_lib.ComponentsFramesArgs), B=B, P=P, H=H, W=W, connectivity=int(connectivity),
                                          min_area=int(min_area), largest=int(bool(largest)), max_runs=int(max_runs), max_components=maxc,
                                          bits=bits.bits.data_ptr(), bits_words=int(bits.bits.numel()), bits_offsets=bits.offsets.data_ptr(),
                                          frames=frames.table.data_ptr() if P else None, image_index=ii.data_ptr(),
                                          out_bits=None if out is None else out.data_ptr(), out_words=0 if out is None else int(out.numel()),
                                          out_offsets=None if out is None else bits.offsets.data_ptr(),
                                          stats=None if stats is None else stats.data_ptr(), components=None if comps is None else comps.data_ptr(),
                                          workspace=ws.data_ptr(), stream=_stream(stream))
            check(lib.la3d_components_bits_frames(C.byref(a)), "la3d_components_bits_frames")
    _record(stream, bits.bits, bits.offsets, frames.table, ii, out, stats, comps, ws)
    return stats, comps


def components_bits_frames(frames, bits: FrameBits, min_area: int = 0, largest: bool = False, connectivity: int = 8, max_components: int = 0,
                           max_runs: int = 16384, stream=None, out=None, return_stats: bool = False):
    """``components_bits`` for the planes of images of DIFFERENT sizes in one call (C-ABI ``la3d_components_bits_frames``): every plane
    of ``bits`` labelled over its OWN image, the kept components written in the input's geometry.  ``frames``: a ``PackedFrames`` /
    ``PackedFrames16`` / ``PackedLabels`` / ``PackedMasks`` / ``FrameGrid`` whose frame table the planes were laid out for (another
    table: ValueError before any device work); ``min_area`` / ``largest`` / ``connectivity`` / ``max_components`` / ``max_runs`` as in
    ``components_bits``, ONE of each per call.  ``out``: a flat, 16-byte aligned int32 device tensor of at least ``bits.bits.numel()``
    words to fill; it must not overlap ``bits.bits`` (the call cannot work in place).  Returns ``FrameBits(out, bits.offsets,
    bits.image_index, area, bits.table, bits.H, bits.W)`` - the planes lie where the input's lie in their buffer, the offsets tensor is
    shared, ``area`` is the kept area -, which goes straight into ``fit_instances_frames_bits``, ``instance_points_frames``,
    ``rle_encode_bits_frames``, ``open_bits_frames`` and ``mask_overlap`` with the same ``frames``; or ``(FrameBits, stats)`` with
    ``return_stats``, or ``(FrameBits, stats, components)`` when ``max_components > 0`` - ``stats`` int32 (B, 8) and ``components``
    int32 (B, max_components, 5) as in ``components_bits``.  A plane with more than ``max_runs`` runs gets ``stats = -1, runs, 0, ...``
    and an all-zero plane; a row whose image index, frame row or plane offset breaks the contract, or whose plane does not end inside
    its buffer, writes no word and gets ``stats = -2, 0, ...`` (``area`` 0 in the ``FrameBits``) - decided on the device, never an
    exception.  No host synchronisation and no host copy of the image indices; capturable."""
    who = "components_bits_frames"
    _components_frames_check(who, frames, bits, min_area, largest, connectivity, max_components, max_runs)
    total = int(bits.bits.numel())
    _flat_out(who, out, total, bits.bits)
    dev = _on_gpu(frames.table, bits.bits)
    if out is not None and out.device != dev:
        raise ValueError(f"{who}: out lives on another device")
    with torch.cuda.device(dev):
        o = torch.empty(max(total, 4), dtype=torch.int32, device=dev) if out is None else out
        stats, comps = _components_frames_run(frames, bits, min_area, largest, connectivity, max_components, max_runs, o, True, stream)
        area = torch.empty(int(stats.shape[0]), dtype=torch.int32, device=dev)
        with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):   # behind the kernel, on ITS stream
            torch.clamp(stats[:, 3], min=0, out=area)
    _record(stream, area)
    res = FrameBits(o, bits.offsets, bits.image_index, area, bits.table, bits.H, bits.W)
    if int(max_components) > 0:
        return res, stats, comps
    return (res, stats) if return_stats else res


def components_stats_frames(frames, bits: FrameBits, min_area: int = 0, largest: bool = False, connectivity: int = 8, max_components: int = 0,
                            max_runs: int = 16384, stream=None):
    """The statistics of ``components_bits_frames`` without its planes (``out_bits = NULL``: nothing but the planes is read): ``stats``
    int32 (B, 8), or ``(stats, components)`` when ``max_components > 0``."""
    who = "components_stats_frames"
    _components_frames_check(who, frames, bits, min_area, largest, connectivity, max_components, max_runs)
    _on_gpu(frames.table, bits.bits)
    stats, comps = _components_frames_run(frames, bits, min_area, largest, connectivity, max_components, max_runs, None, True, stream)
    return (stats, comps) if int(max_components) > 0 else stats


def largest_component_bits_frames(frames, bits: FrameBits, connectivity: int = 8, min_area: int = 0, max_runs: int = 16384, stream=None,
                                  out=None, return_stats: bool = False):
    """The largest connected component of every plane of a shard (``components_bits_frames(largest=True)``): one object per instance
    before ``fit_instances_frames_bits`` takes every set pixel."""
    return components_bits_frames(frames, bits, min_area=min_area, largest=True, connectivity=connectivity, max_runs=max_runs, stream=stream,
                                  out=out, return_stats=return_stats)


def drop_islands_bits_frames(frames, bits: FrameBits, min_area: int, connectivity: int = 8, max_runs: int = 16384, stream=None, out=None,
                             return_stats: bool = False):
    """Every plane of a shard without its components of fewer than ``min_area`` pixels (``components_bits_frames(min_area=...)``)."""
    return components_bits_frames(frames, bits, min_area=min_area, largest=False, connectivity=connectivity, max_runs=max_runs, stream=stream,
                                  out=out, return_stats=return_stats)
