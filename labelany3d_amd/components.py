"""Connected components on bit planes (include/la3d.h "connected components on bit planes"): keep the largest part of every mask, or
drop its islands under an area, on the GPU - ``scipy.ndimage.label`` + ``np.bincount`` for a batch of ``MaskBits`` without the unpack /
device-to-host copy / pack round trip.  ``components_bits`` is the general form; ``largest_component_bits`` and ``drop_islands_bits``
are its two thin forms, ``components_stats`` the statistics-only call."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .batched import _bits_stride, _record, _stream
from .bits import MaskBits, _bits_out, _mask_bits


def _int_arg(who: str, name: str, v, lo: int, hi=None) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < lo or (hi is not None and int(v) > hi):
        rng = f">= {lo}" if hi is None else f"in {lo} .. {hi}"
        raise ValueError(f"{who}: {name} must be an int {rng}, not {v!r}")
    return int(v)


def _components_args(who: str, bits, min_area, largest, connectivity, max_components, max_runs) -> MaskBits:
    if not isinstance(bits, MaskBits):
        raise ValueError(f"{who}: bits must be a MaskBits (pack_mask_bits, pack_rle_bits, pack_poly_bits, pack_crop_bits, ...)")
    _int_arg(who, "min_area", min_area, 0)
    if not isinstance(largest, (bool, np.bool_)) and not (isinstance(largest, (int, np.integer)) and int(largest) in (0, 1)):
        raise ValueError(f"{who}: largest must be a bool, not {largest!r}")
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or int(connectivity) not in (4, 8):
        raise ValueError(f"{who}: connectivity must be 4 or 8, not {connectivity!r}")
    _int_arg(who, "max_components", max_components, 0)
    _int_arg(who, "max_runs", max_runs, 1, _lib.COMPONENTS_MAX_RUNS)
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
