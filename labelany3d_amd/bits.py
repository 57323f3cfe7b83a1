"""Masks as bit planes of ONE frame size per call (include/la3d.h "masks as bit planes" and what followed it): ``MaskBits``, the packers
(u8 masks, logits, run lengths, polygons), the restore of crop-space masks, the unpacker and the plane statistics, the depth gate
(``gate_depth_bits``) and the fit that takes the planes (``fit_instances_bits``).  ``labels`` builds on this module; mixed-size packers: ``frames``; plane operations: ``morph``, ``rle_encode``."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._device import _as_dev, _dev, _plane_source, _ptr, _record, _stream, _upload_many
from ._lib import check, lib
from .batched import Depth16, _bits_stride, _depth16_check, height_rule_code, padded_width
from .fitcall import depth_rows_for_bits, fit_call, mask_source
from .segm import pack_rle


class MaskBits(NamedTuple):
    """Masks as bit planes (include/la3d.h "masks as bit planes"): ``bits`` int32 (B, words) on the GPU - row b holds the
    ``ceil(H*W/32)`` little-endian words of plane b, pixel (v, u) = bit ``(v*W + u) & 31`` of word ``(v*W + u) >> 5``, i.e.
    ``np.packbits(mask.reshape(B, -1), axis=1, bitorder="little")`` viewed as uint32 -; ``H``, ``W``: the frame as STORED (rows
    padded to ``W``); ``frame_width``: the image columns (== W when the rows are not padded)."""
    bits: torch.Tensor
    H: int
    W: int
    frame_width: int


def _mask_bits(bits) -> MaskBits:
    if not (isinstance(bits, tuple) and len(bits) == 4):
        raise ValueError("bits must be the (bits, H, W, frame_width) tuple of pack_mask_bits / pack_logits_bits")
    mb = MaskBits(bits[0], int(bits[1]), int(bits[2]), int(bits[3]))
    if not 0 < mb.frame_width <= mb.W:
        raise ValueError("frame_width must lie in (0, W]")
    _bits_stride(mb.bits, mb.bits.shape[0] if isinstance(mb.bits, torch.Tensor) and mb.bits.dim() == 2 else 0, mb.H, mb.W)
    return mb


def _bits_out(out, B, H, W_out, dev):
    nwords = (H * W_out + 31) // 32
    if out is None:
        return torch.empty((B, nwords), dtype=torch.int32, device=dev)
    _bits_stride(out, B, H, W_out)
    return out


def pack_mask_bits(masks, frame_pad: bool = True, device=None, stream=None, out=None) -> MaskBits:
    """(B,H,W) bool / uint8 masks (non-zero = True) -> ``MaskBits`` on the GPU (C-ABI ``la3d_pack_mask_bits``).  ``frame_pad``: rows
    of a width that is not a multiple of 32 are padded with zero bits to ``padded_width(W)`` - exactly as ``pad_depth_rows`` pads
    the depth -, which is what the tiled forms of the fit want (``frame_width`` of the result keeps W).  A device tensor with
    dense planes is read in place (any plane stride, any base alignment).  ``out``: an int32 (B, >= words) device tensor to fill
    (only the words of each plane are written).  Worth it when the masks are fitted more than once or stay resident: a single
    fit of a u8 plane that already exists reads fewer bytes through ``fit_instances``."""
    if device is None and isinstance(masks, torch.Tensor) and masks.is_cuda:
        device = masks.device
    dev = _dev(device)
    m, ps = _plane_source(masks, dev, (torch.uint8, torch.bool))
    B, H, W = m.shape
    W_out = padded_width(W) if frame_pad else W
    o = _bits_out(out, B, H, W_out, dev)
    with torch.cuda.device(dev):
        check(lib.la3d_pack_mask_bits(_ptr(m), ps, B, H, W, W_out, _ptr(o), _bits_stride(o, B, H, W_out), _stream(stream)),
              "la3d_pack_mask_bits")
    _record(stream, m, o)
    return MaskBits(o, H, W_out, W)


_LOGIT_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}


def pack_logits_bits(logits, threshold: float = 0.0, frame_pad: bool = True, device=None, stream=None, out=None) -> MaskBits:
    """(B,H,W) float32 / float16 / bfloat16 logits of a segmentation network -> ``MaskBits`` of ``logits > threshold`` (compared in
    float32; NaN -> 0), without a boolean plane in between (C-ABI ``la3d_pack_logits_bits``).  Other arguments as
    ``pack_mask_bits``."""
    if device is None and isinstance(logits, torch.Tensor) and logits.is_cuda:
        device = logits.device
    dev = _dev(device)
    x, ps = _plane_source(logits, dev, (torch.float32, torch.float16, torch.bfloat16))
    B, H, W = x.shape
    W_out = padded_width(W) if frame_pad else W
    o = _bits_out(out, B, H, W_out, dev)
    with torch.cuda.device(dev):
        check(lib.la3d_pack_logits_bits(_ptr(x), _LOGIT_DTYPES[x.dtype], ps, float(threshold), B, H, W, W_out, _ptr(o),
                                        _bits_stride(o, B, H, W_out), _stream(stream)), "la3d_pack_logits_bits")
    _record(stream, x, o)
    return MaskBits(o, H, W_out, W)


def _annotation_bits_plan(who, B, H, W, frame_pad, device, out, area):
    """The argument errors of ``pack_rle_bits`` / ``pack_poly_bits`` that need no device -> (W_out, the plane stride of ``out`` or None,
    the device to ask for).  ``out`` is checked ONCE, here: at small batches the packers are bound by what this wrapper costs."""
    if B and (H <= 0 or W <= 0):
        raise ValueError(f"{who}: the annotations state an empty frame {(H, W)}")
    W_out = padded_width(W) if frame_pad else W
    stride = None if out is None else _bits_stride(out, B, H, W_out)
    if area is not None and not (isinstance(area, torch.Tensor) and area.is_cuda and area.dtype == torch.int32 and area.dim() == 1
                                 and area.numel() == B and area.is_contiguous()):
        raise ValueError(f"{who}: area must be a contiguous int32 ({B},) tensor on the GPU")
    where = out.device if out is not None else area.device if area is not None else None
    if where is not None:
        d = where if device is None else torch.device(device)   # ("cuda" without an index names whichever GPU the tensors are on)
        if (area is not None and area.device != where) or d.type != where.type or (d.index is not None and d.index != where.index):
            raise ValueError(f"{who}: out / area live on another device")
    return W_out, stride, where if where is not None else device


class _PackedBits(MaskBits):
    """The ``MaskBits`` a packer of annotations returns: it has just checked and filled the planes, so ``_stride`` - their plane
    stride in words - rides along and a consumer (``instance_points``) need not check the tensor again.  A tuple like any
    ``MaskBits``; ``_replace`` gives one without the attribute, which is checked as usual."""


def _pack_annotation_bits(entry, name, arrays, B, H, W, frame_pad, device, stream, out, area) -> MaskBits:
    """What ``pack_rle_bits`` / ``pack_poly_bits`` share: the checks, the planes, the annotation arrays (resident tensors as they are,
    host arrays in one copy), the call.  At small batches the call costs what this wrapper costs: nothing is checked twice, and the
    device context is entered only when another device is current."""
    W_out, stride, device = _annotation_bits_plan(name[5:], B, H, W, frame_pad, device, out, area)
    dev = device if isinstance(device, torch.device) else _dev(device)
    if out is None:
        stride = (H * W_out + 31) // 32
        out = torch.empty((B, stride), dtype=torch.int32, device=dev)
    if B:
        # (the device context costs ~1.5 us of the ~12 us this call costs at small batches: entered only when another device is current)
        with contextlib.nullcontext() if torch.cuda.current_device() == dev.index else torch.cuda.device(dev):
            ann = []
            for a, dt in arrays:   # (resident arrays of the right dtype are taken as they are)
                if not (isinstance(a, torch.Tensor) and a.dtype == dt and a.device == dev and a.is_contiguous()):
                    ann = None
                    break
                ann.append(a)
            if ann is None:
                ann = ([_as_dev(a, dt, dev) for a, dt in arrays] if any(isinstance(a, torch.Tensor) for a, _ in arrays)
                       else _upload_many(arrays, dev))
            # (plain integers: the entries' pointer arguments are c_void_p)
            check(entry(*[a.data_ptr() for a in ann], B, H, W, W_out, out.data_ptr(), stride, None if area is None else area.data_ptr(),
                        _stream(stream)), name)
        _record(stream, *ann, out, area)
    mb = _PackedBits(out, H, W_out, W)
    mb._stride = stride
    return mb


def pack_rle_bits(rles, frame_pad: bool = True, device=None, stream=None, out=None, area=None) -> MaskBits:
    """COCO run lengths (a list of RLE objects or the tuple of ``pack_rle``) -> ``MaskBits`` on the GPU (C-ABI ``la3d_pack_rle_bits``):
    ``rle_decode`` with the bit image kept - an eighth of the bytes of the boolean planes, what ``instance_points``,
    ``mask_stats_bits``, ``unpack_mask_bits`` and ``fit_instances_bits`` take.  ``frame_pad`` / ``out`` as in ``pack_mask_bits``;
    ``area``: an int32 (B,) device tensor that receives the popcount of every plane (what ``area_hint`` takes).  A negative count is
    a run of length 0, runs past the frame are cut."""
    counts, offsets, H, W = pack_rle(rles)
    return _pack_annotation_bits(lib.la3d_pack_rle_bits, "la3d_pack_rle_bits", [(counts, torch.int32), (offsets, torch.int64)],
                                 len(offsets) - 1, H, W, frame_pad, device, stream, out, area)


def pack_poly_bits(polys, frame_pad: bool = True, device=None, stream=None, out=None, area=None) -> MaskBits:
    """Polygon parts (the tuple of ``pack_polygons``) -> ``MaskBits`` on the GPU (C-ABI ``la3d_pack_poly_bits``): ``poly_decode``
    with the bit image kept.  Other arguments as ``pack_rle_bits``."""
    if not (isinstance(polys, tuple) and len(polys) == 5):
        raise ValueError("polys must be the (xy, ring_offsets, inst_rings, H, W) tuple of pack_polygons")
    return _pack_annotation_bits(lib.la3d_pack_poly_bits, "la3d_pack_poly_bits",
                                 [(polys[0], torch.int32), (polys[1], torch.int64), (polys[2], torch.int64)], len(polys[2]) - 1,
                                 int(polys[3]), int(polys[4]), frame_pad, device, stream, out, area)


# ---- crop-space masks as bit planes (include/la3d.h "crop-space masks as bit planes") -----------------------------------------------
def crop_placement(params, S: int) -> np.ndarray:
    """The paste of ``restore_mask_from_crop`` (reference src/util.py:187, :196-197) for a batch of crops of side ``S``: ``params``
    (B, 3) or a list of ``(offset_x, offset_y, scale_factor)`` -> int32 (B, 4) rows ``x1, y1, side, 0`` - what ``la3d_pack_crop_bits``
    reads as ``place``.  Host arithmetic on Python floats, exactly the reference's: ``side = int(S / scale_factor)`` (truncated),
    ``x1 = int(round(offset_x))`` with Python's ``round`` (half to even); a scale of 0 and values that are no numbers raise what they
    raise there.  Values that do not fit an int32 are clamped (such a placement lies outside every frame, such a side is refused on
    the device: an empty plane)."""
    rows = params.tolist() if hasattr(params, "tolist") else list(params)
    out = np.zeros((len(rows), 4), np.int32)
    lim = 2 ** 31 - 1
    for n, row in enumerate(rows):
        if len(row) != 3:
            raise ValueError(f"crop_placement: row {n} must be (offset_x, offset_y, scale_factor)")
        ox, oy, s = (float(v) for v in row)
        out[n, :3] = [max(-lim, min(lim, i)) for i in (int(round(ox)), int(round(oy)), int(int(S) / s))]
    return out


def _crop_source(who, crops, dev):
    """``crops`` of a crop packer -> (tensor that owns the bytes, the view whose first byte is crop 0's pixel (0, 0), crop stride, row
    pitch, pixel step - bytes -, S, B, the default threshold).  (B, S, S) bool / uint8: a mask, threshold 0; (B, S, S, 4) uint8: RGBA,
    the alpha channel is read in place through the strides, threshold 127 (reference src/batch_scripts/whole.py:83).  A device tensor
    is read where it lies when a crop's rows and pixels lie at non-negative strides that do not overlap; host arrays go up as the
    S x S bytes that are read."""
    shape = tuple(crops.shape) if hasattr(crops, "shape") else None
    if shape is None:
        crops = np.asarray(crops)
        shape = crops.shape
    rgba = len(shape) == 4
    if not ((len(shape) == 3 or (rgba and shape[3] == 4)) and shape[1] == shape[2] and shape[1] > 0):
        raise ValueError(f"{who}: crops must be (B, S, S) bool / uint8 masks or (B, S, S, 4) uint8 RGBA crops, got {shape}")
    B, S = int(shape[0]), int(shape[1])
    if isinstance(crops, torch.Tensor):
        if crops.dtype not in ((torch.uint8,) if rgba else (torch.uint8, torch.bool)):
            raise ValueError(f"{who}: crops must be uint8{'' if rgba else ' or bool'}, not {crops.dtype}")
        t = crops.view(torch.uint8) if crops.dtype == torch.bool else crops
        v = t[..., 3] if rgba else t
        if v.device != dev:
            v = v.to(dev)
        sb, sr, sp = v.stride()
        if not (sp >= 1 and sr >= S * sp and (B <= 1 or sb >= (S - 1) * sr + (S - 1) * sp + 1)):
            v = v.contiguous()
            sb, sr, sp = v.stride()
    else:
        a = np.asarray(crops)
        if a.dtype not in ((np.uint8,) if rgba else (np.uint8, np.bool_)):
            raise ValueError(f"{who}: crops must be uint8{'' if rgba else ' or bool'}, not {a.dtype}")
        a = np.ascontiguousarray(a[..., 3] if rgba else a).view(np.uint8)
        v = torch.as_tensor(a, device=dev)
        sb, sr, sp = S * S, S, 1
    if B <= 1:
        sb = max(int(sb), (S - 1) * int(sr) + (S - 1) * int(sp) + 1)
    return v, int(sb), int(sr), int(sp), S, B, (127 if rgba else 0)


def _crop_threshold(who, threshold, default: int) -> int:
    thr = default if threshold is None else int(threshold)
    if not 0 <= thr <= 255:
        raise ValueError(f"{who}: threshold must lie in [0, 255] (bit = byte > threshold)")
    return thr


def _crop_place(who, params, S: int, B: int, dev) -> torch.Tensor:
    """``params`` of a crop packer -> the int32 (B, 4) ``place`` rows on the device: host parameters through ``crop_placement``; an
    int32 (B, 4) device tensor is taken as the rows themselves (``crop_placement`` uploaded once: nothing is copied, the call is
    capturable)."""
    if isinstance(params, torch.Tensor) and params.is_cuda:
        if not (params.dtype == torch.int32 and tuple(params.shape) == (B, 4) and params.is_contiguous() and params.device == dev):
            raise ValueError(f"{who}: device params must be the contiguous int32 ({B}, 4) rows of crop_placement, on the crops' device")
        return params
    place = crop_placement(params, S)
    if len(place) != B:
        raise ValueError(f"{who}: params must hold one (offset_x, offset_y, scale_factor) per crop ({B}), got {len(place)}")
    return torch.as_tensor(place, device=dev)


def pack_crop_bits(crops, params, image_size, threshold=None, frame_pad: bool = True, device=None, stream=None, out=None,
                   area=None) -> MaskBits:
    """Crop-space masks -> ``MaskBits`` of the full frame on the GPU (C-ABI ``la3d_pack_crop_bits``): ``restore_mask_from_crop``
    (reference src/util.py:171-214) for a batch, written as bit planes - the nearest-index resize to ``int(S / scale_factor)`` pixels
    and the clipped paste at ``round(offset)`` happen inside one kernel, so a 640x480 instance costs its 65 536 B crop (nothing when
    the crop is resident) instead of a host resize, a 307 200 B upload and a pack.  ``crops``: (B, S, S) bool / uint8 masks (bit =
    byte > ``threshold``, default 0) or (B, S, S, 4) uint8 RGBA crops, whose alpha is read in place (default threshold 127, as at
    src/batch_scripts/whole.py:83), on the host or the device; ``params``: (B, 3) ``(offset_x, offset_y, scale_factor)`` as
    ``crop_object`` returns them (``crop_placement`` turns them into the paste on the host, in the reference's float arithmetic), or
    the int32 (B, 4) rows of ``crop_placement`` already on the device (nothing is uploaded then: with resident crops the call copies
    nothing and can be captured into a graph);
    ``image_size`` = (width, height).  ``frame_pad`` / ``out`` / ``area`` as in ``pack_rle_bits``.  Unlike the reference, a scale
    that leaves no pixel (side <= 0) and a crop that lies wholly outside the frame give an empty plane (area 0), not an exception."""
    who = "pack_crop_bits"
    if device is None and isinstance(crops, torch.Tensor) and crops.is_cuda:
        device = crops.device
    W, H = int(image_size[0]), int(image_size[1])
    B0 = int(crops.shape[0]) if hasattr(crops, "shape") else len(crops)
    W_out, stride, device = _annotation_bits_plan(who, B0, H, W, frame_pad, device, out, area)
    if H <= 0 or W <= 0:
        raise ValueError(f"{who}: image_size states an empty frame {(W, H)}")
    dev = device if isinstance(device, torch.device) else _dev(device)
    with torch.cuda.device(dev):
        v, sb, sr, sp, S, B, default = _crop_source(who, crops, dev)
        thr = _crop_threshold(who, threshold, default)
        place = _crop_place(who, params, S, B, dev)
        if out is None:
            stride = (H * W_out + 31) // 32
            out = torch.empty((B, stride), dtype=torch.int32, device=dev)
        check(lib.la3d_pack_crop_bits(v.data_ptr(), sb, sr, sp, S, thr, place.data_ptr(), B, H, W, W_out, out.data_ptr(), stride,
                                      None if area is None else area.data_ptr(), _stream(stream)), "la3d_pack_crop_bits")
    _record(stream, v, place, out, area)
    mb = _PackedBits(out, H, W_out, W)
    mb._stride = stride
    return mb


def unpack_mask_bits(bits, stream=None) -> torch.Tensor:
    """``MaskBits`` -> (B,H,frame_width) bool masks on the GPU (C-ABI ``la3d_unpack_mask_bits``)."""
    mb = _mask_bits(bits)
    B = mb.bits.shape[0]
    out = torch.empty((B, mb.H, mb.frame_width), dtype=torch.uint8, device=mb.bits.device)
    with torch.cuda.device(mb.bits.device):
        check(lib.la3d_unpack_mask_bits(_ptr(mb.bits), _bits_stride(mb.bits, B, mb.H, mb.W), B, mb.H, mb.W, mb.frame_width, _ptr(out),
                                        _stream(stream)), "la3d_unpack_mask_bits")
    _record(stream, mb.bits, out)
    return out.view(torch.bool)


def mask_stats_bits(bits, boundary_threshold: int = 10, stream=None) -> torch.Tensor:
    """``mask_stats`` of ``MaskBits``: (B,4) int32 - area, rows holding a pixel, last - first + 1 rows, boundary-strip pixels (the
    right strip ends at ``frame_width``)."""
    mb = _mask_bits(bits)
    B = mb.bits.shape[0]
    out = torch.empty((B, 4), dtype=torch.int32, device=mb.bits.device)
    with torch.cuda.device(mb.bits.device):
        check(lib.la3d_mask_stats_bits(_ptr(mb.bits), _bits_stride(mb.bits, B, mb.H, mb.W), B, mb.H, mb.W, mb.frame_width,
                                       int(boundary_threshold), _ptr(out), _stream(stream)), "la3d_mask_stats_bits")
    _record(stream, mb.bits, out)
    return out


# ---- the depth gate (include/la3d.h "depth gate on bit planes") -----------------------------------------------------------------------
class DepthGateStats(NamedTuple):
    """What ``gate_depth_bits`` / ``depth_gate_stats`` say about every plane, on the GPU: ``counts`` int32 (B, 3) = ``area_in`` (set
    pixels of the image columns), ``n_valid`` (of them, those whose depth is finite and inside ``[near, far]``), ``area_out`` (kept);
    ``levels`` float32 (B, 3) = ``med, mad, thr`` (NaN where no pixel is valid)."""
    counts: torch.Tensor
    levels: torch.Tensor


def _gate_level(who: str, name: str, v, default: float) -> float:
    """``near`` / ``far``: None (no bound) or a real number that is not NaN -> the float the block takes."""
    if v is None:
        return default
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v:
        raise ValueError(f"{who}: {name} must be None or a number that is not NaN, not {v!r}")
    return float(v)


def _gate_band(who: str, name: str, v) -> float:
    """``k`` / ``min_band``: a real number that is finite and >= 0 as a float32."""
    ok = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))
    with np.errstate(over="ignore"):
        ok = ok and bool(np.isfinite(np.float32(v))) and v >= 0
    if not ok:
        raise ValueError(f"{who}: {name} must be a finite number >= 0, not {v!r}")
    return float(v)


def _gate_run(who: str, depth, bits, k, min_band, near, far, image_index, stream, out, want_plane: bool, want_stats: bool):
    """The checks of ``gate_depth_bits`` / ``depth_gate_stats`` and one ``la3d_depth_gate_bits`` call -> (MaskBits or None, stats or None)."""
    if not isinstance(bits, MaskBits):
        raise ValueError(f"{who}: bits must be a MaskBits (pack_mask_bits, pack_rle_bits, pack_poly_bits, pack_crop_bits, ...)")
    k, min_band = _gate_band(who, "k", k), _gate_band(who, "min_band", min_band)
    near, far = _gate_level(who, "near", near, float("-inf")), _gate_level(who, "far", far, float("inf"))
    if isinstance(depth, Depth16):
        raise ValueError(f"{who}: depth must be float32 planes, not a Depth16 (unpack_depth16 gives them)")
    dtype = depth.dtype if isinstance(depth, torch.Tensor) else np.asarray(depth).dtype
    if dtype not in (torch.float32, np.dtype(np.float32)):
        raise ValueError(f"{who}: depth must be float32, not {dtype}")
    mb = _mask_bits(bits)
    B, H, W, fw, dev = int(mb.bits.shape[0]), mb.H, mb.W, mb.frame_width, mb.bits.device
    if H <= 0 or W <= 0:
        raise ValueError(f"{who}: the planes state an empty frame {(H, W)}")
    if H * W > _lib.DEPTH_GATE_MAX_PIXELS:
        raise ValueError(f"{who}: a frame of {(H, W)} has more than {_lib.DEPTH_GATE_MAX_PIXELS} stored pixels")
    for name, t in (("depth", depth), ("image_index", image_index), ("out", out)):
        if isinstance(t, torch.Tensor) and t.is_cuda and t.device != dev:
            raise ValueError(f"{who}: {name} lives on another device than the bit planes")
    shape = tuple(depth.shape)
    if len(shape) not in (2, 3) or shape[-2] != H:
        raise ValueError(f"{who}: depth {shape} must be (H, W), (P, H, W) or (B, H, W) planes of {H} rows")
    P = 1 if len(shape) == 2 else int(shape[0])
    if image_index is None:
        if P not in (1, B):
            raise ValueError(f"{who}: {P} depth planes for {B} instances need an image_index")
    elif tuple(image_index.shape) != (B,):
        raise ValueError(f"{who}: image_index must be (B,)")
    elif not (isinstance(image_index, torch.Tensor) and image_index.is_cuda) and B:   # (a device index is not read back)
        host = np.asarray(image_index)
        if host.min() < 0 or host.max() >= P:
            raise ValueError(f"{who}: image_index must lie in [0, {P})")
    o = _bits_out(out, B, H, W, dev) if want_plane else None
    with torch.cuda.device(dev):
        d, _ = depth_rows_for_bits(depth, W, fw, dev)
        d = _as_dev(d, torch.float32, dev)
        ii = None if image_index is None else _as_dev(image_index, torch.int32, dev)
        counts = torch.empty((B, 3), dtype=torch.int32, device=dev) if want_stats else None
        levels = torch.empty((B, 3), dtype=torch.float32, device=dev) if want_stats else None
        if B:   # (an empty batch has no planes to point at)
            a = _lib.DepthGateArgs(struct_size=C.sizeof(_lib.DepthGateArgs), B=B, H=H, W=W, frame_width=0 if fw == W else fw,
                                   k=k, min_band=min_band, near=near, far=far, depth=d.data_ptr(), depth_plane_stride=0 if P == 1 else H * W,
                                   image_index=None if ii is None else ii.data_ptr(),
                                   mask_bits=mb.bits.data_ptr(), bits_plane_stride=_bits_stride(mb.bits, B, H, W),
                                   out_bits=None if o is None else o.data_ptr(), out_plane_stride=0 if o is None else _bits_stride(o, B, H, W),
                                   counts=None if counts is None else counts.data_ptr(), levels=None if levels is None else levels.data_ptr(),
                                   stream=_stream(stream))
            check(lib.la3d_depth_gate_bits(C.byref(a)), "la3d_depth_gate_bits")
    _record(stream, d, ii, mb.bits, o, counts, levels)
    return (None if o is None else MaskBits(o, H, W, fw)), (DepthGateStats(counts, levels) if want_stats else None)


def gate_depth_bits(depth, bits: MaskBits, k: float = 4.5, min_band: float = 0.0, near=None, far=None, image_index=None, stream=None,
                    out=None, return_stats: bool = False):
    """Drop every mask's depth outliers before ``fit_instances_bits`` takes every set pixel (C-ABI ``la3d_depth_gate_bits``): the
    fit's extents are plain minima and maxima, so one fill value of the depth stage (the reference's ``align_depth`` writes 10000.0)
    or a few background pixels behind an occlusion edge set the size of the box.  Per plane, with ``d`` its depth plane:
    ``valid = m & isfinite(d) & (d >= near) & (d <= far)``, ``med = np.median(d[valid])``, ``mad = np.median(|d[valid] - med|)``,
    ``thr = max(k * mad, min_band)``, ``keep = valid & (|d - med| <= thr)`` - all in float32, the medians exact (an even count
    averages the two middle values).  ``k``: the band in MADs (4.5 is about three sigma of a Gaussian; a surface whose depths are
    spread uniformly over their range keeps every pixel); ``min_band``: a floor for the band in depth units - needed where quantised
    depth gives ``mad == 0``, which otherwise keeps only the pixels exactly at the median; ``near`` / ``far``: None, or the depths
    that count at all (``far=9999`` handles the reference's fill by itself).  A plane without a valid pixel comes back empty, with NaN
    levels.  ``depth``: float32 - (H, W) shared by every plane, (P, H, W) with ``image_index`` (B,), or (B, H, W) -, as wide as the
    planes are stored (``bits.W``) or ``bits.frame_width`` wide - then the rows are padded here, as ``fit_instances_bits`` does; a
    ``Depth16`` or another dtype is refused.  ``out``: None (a fresh tensor), an int32 (B, >= words) device tensor to fill, or
    ``bits.bits`` itself (in place); any other overlap with the input is refused.  Returns the ``MaskBits`` of the kept pixels in the
    input's geometry (pad columns and tail bits zero whatever the input held there) - or ``(MaskBits, DepthGateStats)`` with
    ``return_stats``.  One kernel, no host synchronisation; capturable."""
    res, stats = _gate_run("gate_depth_bits", depth, bits, k, min_band, near, far, image_index, stream, out, True, bool(return_stats))
    return (res, stats) if return_stats else res


def depth_gate_stats(depth, bits: MaskBits, k: float = 4.5, min_band: float = 0.0, near=None, far=None, image_index=None,
                     stream=None) -> DepthGateStats:
    """The ``DepthGateStats`` of ``gate_depth_bits`` without its planes (``out_bits = NULL``: no plane is written)."""
    return _gate_run("depth_gate_stats", depth, bits, k, min_band, near, far, image_index, stream, None, False, True)[1]


def fit_instances_bits(depth, bits, K, ground=None, sample_idx=None, image_index=None, stream=None, device=None, filter=None,
                       image_size=None, area_hint=None, frame_width=None, method: str = "pca", height_rule: str = "rows"):
    """fit_instances with the masks given as bit planes (``pack_mask_bits`` / ``pack_logits_bits``; C-ABI
    ``la3d_fit_instances_bits``): the planes are copied straight into the fit kernel's LDS bit image - an eighth of the bytes of a u8
    plane, no decode.  Arguments and returns as ``fit_instances_rle`` (``filter`` adds the (B,4) statistics), plus ``image_size`` /
    ``area_hint`` as in ``fit_instances_ex`` (``image_size`` appends ``boxes2d`` (B,8) to the returned tuple).  ``depth``: planes as
    wide as the bit planes are stored (``bits.W``), or ``bits.frame_width`` wide - then the rows are padded here
    (``pad_depth_rows``).  ``frame_width``: None, or the image width, checked against the planes'.  ``height_rule``: the height the
    fused filter uses - "rows" (rows holding a pixel, the reference's rule for run-length annotations) or "span" (last - first + 1,
    its rule for polygons); a bit plane does not say where it came from."""
    _lib.method_code(method)   # (the reference's error for an unknown method, before any device work)
    flags = height_rule_code(height_rule)
    if isinstance(depth, Depth16):
        _depth16_check(depth)
    mb = _mask_bits(bits)
    dev = mb.bits.device if device is None else _dev(device)
    if mb.bits.device != dev:
        raise ValueError("the bit planes live on another device")
    W, fw = mb.W, mb.frame_width
    if frame_width is not None and int(frame_width) != fw:
        raise ValueError(f"frame_width {frame_width} does not match the bit planes' frame width {fw}")
    depth, fw = depth_rows_for_bits(depth, W, fw, dev)
    out = fit_call(mask_source(dev, bits=(mb, flags))[0], depth, K, dev, mb.H, W, image_index=image_index, ground=ground,
                   sample_idx=sample_idx, area_hint=area_hint, filter=filter, image_size=image_size, stream=stream, method=method,
                   frame_width=fw)
    return tuple(out.values())
