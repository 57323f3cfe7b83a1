"""The one place a depth + mask fit call of the convenience wrappers is built (``masks.fit_instances_ex`` / ``fit_instances_bits``,
``frames.fit_instances_frames`` / ``fit_instances_frames_bits``): a mask source, a depth source, the shared input checks, the outputs, the ``la3d_fit_args`` block, the
enqueue, the stream bookkeeping.  A wrapper does its own argument checks, calls ``fit_call`` and shapes what it returns; a new
source is one description here plus the checks that are its own."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib, options
from ._device import _as_dev, _bulk, _ptr, _record, _stream
from .batched import Depth16, InstanceFitter, _bits_stride, _enqueue, _fit_args, _fit_inputs, _pad_rows16, pad_depth_rows, padded_width


class MaskSource(NamedTuple):
    """The masks of a call: ``B`` instances on a frame of ``H`` x ``W`` (None, None: a frames call - every instance has its own);
    ``kw``: the mask keywords of ``_fit_args``; ``bits``: the (pointer, stride, flags) of bit planes - in a frames call (pointer,
    pointer to the per-instance plane offsets, flags); ``keep``: the tensors behind the pointers; ``what``: the word the error texts
    use for the masks."""
    B: int
    H: Optional[int]
    W: Optional[int]
    kw: dict
    bits: Optional[tuple]
    keep: list
    what: str


class FramesDepth(NamedTuple):
    """The depth of a frames call: the flat buffer of a ``PackedFrames`` / ``PackedFrames16``, its device frame table and - 16-bit
    planes - the ``la3d_depth16`` block of the buffer."""
    flat: torch.Tensor
    table: torch.Tensor
    d16: Optional[_lib.Depth16Block]


def mask_source(dev, masks=None, rles=None, polys=None, bits=None, frame_bits=None, small=(None, None, None, None)):
    """-> (MaskSource, ground, image_index, sample_idx, area_hint).  ``masks``: (B,H,W) u8 / bool; ``rles``: (counts, offsets, H, W);
    ``polys``: (xy, ring_offsets, inst_rings, H, W); ``bits``: (``MaskBits``, flags); ``frame_bits``: (``FrameBits``, flags) - the
    bit planes of a frames call, one per instance at its own offset.  Host run-length / polygon arrays go up in ONE
    copy together with the call's other small host arrays ``small`` = (ground, image_index, sample_idx, area_hint), which come back
    as device tensors where they went along (tensors and None pass through)."""
    if masks is not None:
        m = _as_dev(masks, torch.uint8, dev)
        B, H, W = m.shape
        return (MaskSource(B, H, W, dict(mask=_ptr(m)), None, [m], "mask"), *small)
    if bits is not None:
        mb, flags = bits
        B = mb.bits.shape[0]
        return (MaskSource(B, mb.H, mb.W, {}, (_ptr(mb.bits), _bits_stride(mb.bits, B, mb.H, mb.W), flags), [mb.bits], "bit-plane"), *small)
    if frame_bits is not None:
        fb, flags = frame_bits
        return (MaskSource(int(fb.offsets.numel()), None, None, {}, (_ptr(fb.bits), _ptr(fb.offsets), flags), [fb.bits, fb.offsets], "bit-plane"),
                *small)
    i32, i64, (g, ii, si, ah) = torch.int32, torch.int64, small   # (spelled out: this runs once per image on a ~100 us path)
    if rles is not None:
        c, o, H, W = rles
        c, o, g, ii, si, ah = _bulk(dev, (c, i32), (o, i64), (g, torch.float64), (ii, i32), (si, i32), (ah, i32))
        c, o = _as_dev(c, i32, dev), _as_dev(o, i64, dev)
        return MaskSource(o.numel() - 1, H, W, dict(rle=(_ptr(c), _ptr(o))), None, [c, o], "RLE"), g, ii, si, ah
    xy, ro, ir, H, W = polys
    xy, ro, ir, g, ii, si, ah = _bulk(dev, (xy, i32), (ro, i64), (ir, i64), (g, torch.float64), (ii, i32), (si, i32), (ah, i32))
    xy, ro, ir = _as_dev(xy, i32, dev), _as_dev(ro, i64, dev), _as_dev(ir, i64, dev)
    return MaskSource(ir.numel() - 1, H, W, dict(poly=(_ptr(xy), _ptr(ro), _ptr(ir))), None, [xy, ro, ir], "polygon"), g, ii, si, ah


def depth_rows(depth, stored: int, image: int, dev, pad: bool):
    """The depth of a call whose masks are stored ``stored`` pixels wide and hold ``image`` image columns -> (depth, the
    ``frame_width`` to send: 0 when every stored column is image).  ``pad``: the depth rows are ``image`` wide and are padded to
    ``stored`` here (float32: ``pad_depth_rows``; a ``Depth16``: a padded copy of its words); otherwise they are ``stored`` wide
    already."""
    if pad and stored != image:
        with torch.cuda.device(dev):
            if isinstance(depth, Depth16):
                return _pad_rows16(depth, stored), image
            return pad_depth_rows(depth, dev)   # (the image columns as the DEPTH states them, as this route always sent them)
    return depth, (0 if stored == image else image)


def depth_rows_for_bits(depth, stored: int, image: int, dev):
    """``depth_rows`` for bit planes stored ``stored`` pixels wide with ``image`` image columns: depth rows as wide as the planes
    are stored go as they are, rows as wide as the image are padded when that gives the stored width, anything else is refused."""
    Wd = int((depth.data if isinstance(depth, Depth16) else depth).shape[-1])
    if Wd != stored and (Wd != image or padded_width(image) != stored):
        raise ValueError(f"depth rows of {Wd} pixels match neither the stored width {stored} nor the frame width {image} of the bit planes")
    return depth_rows(depth, stored, image, dev, pad=Wd != stored)


def fit_call(src: MaskSource, depth, K, dev, H, W, *, image_index, ground, sample_idx, area_hint, filter, image_size, stream, method,
             frame_width=0, given_index=None, fitter=None, stats=None):
    """Build and enqueue one fit call on a frame of H x W as stored: the shared input checks, the outputs, the area hint, the
    argument block, the C entry, the stream bookkeeping.  -> dict: boxes, status, aux, and stats / boxes2d when asked.
    ``depth``: planes (float32, anything convertible, or a ``Depth16``) - or a ``FramesDepth``: the frames call, which keeps three
    differences of its wrapper as they were: a shared K is not expanded to one matrix per plane, the range of ``image_index`` is
    left to the device (an index outside gives status 5 there, never an exception), and a caller-kept ``fitter`` need only be at
    least as large as the call's bounds (the plane calls want the exact frame).  ``fitter`` / ``stats``: buffers a caller keeps between
    calls instead of allocating them per call (``stats`` is reused by ``fit_annotations`` only)."""
    frames, meth, B = isinstance(depth, FramesDepth), _lib.method_code(method), src.B
    if frames:
        P = int(depth.table.shape[0])
        _, k, ii, g, si, _ = _fit_inputs(None, K, image_index, ground, sample_idx, B, H, W, dev, None, planes=P, expand_K=False,
                                         check_host_index=False)
        H, W = max(int(H), 1), max(int(W), 1)
        d, darg, nplanes, table = depth.flat, depth.d16 if depth.d16 is not None else _ptr(depth.flat), 1, (_ptr(depth.table), P)
    else:
        d, k, ii, g, si, nplanes = _fit_inputs(depth, K, image_index, ground, sample_idx, B, H, W, dev, f"the {src.what} frame",
                                               given_index=given_index)
        darg, table = d if isinstance(d, Depth16) else _ptr(d), None
    out = {}
    with torch.cuda.device(dev):
        f = fitter if fitter is not None else InstanceFitter(B, H, W, dev, method=method)
        boxes, status, aux = f.boxes[0], f.status[0], f.aux[0]
        if fitter is not None:
            wrong_frame = (f.H < H or f.W < W) if frames else (f.H, f.W) != (H, W)
            if f.B < B or wrong_frame or (meth != f.method and meth != _lib.METHOD_PCA):
                raise ValueError("_fitter too small for this call")
        if f.B == B:
            out.update(boxes=boxes, status=status, aux=aux)
        else:   # (a kept fitter may have more rows than this call)
            out.update(boxes=boxes[:B], status=status[:B], aux=aux[:B])
        if filter:
            out["stats"] = stats if stats is not None else torch.zeros((B, 4), dtype=torch.int32, device=dev)
        if image_size is not None:
            out["boxes2d"] = torch.full((B, 8), float("nan"), dtype=torch.float64, device=dev)
        if B == 0:
            return out
        ah = None
        if area_hint is not None:
            ah = _as_dev(area_hint, torch.int32, dev).reshape(-1)
            if ah.numel() != B:
                raise ValueError("area_hint must have one entry per instance")
        a = _fit_args(B, H, W, darg, nplanes, _ptr(k), k.shape[0], _ptr(boxes), _ptr(status), _ptr(aux),
                      _ptr(f.workspace[0]), _stream(stream), image_index=_ptr(ii), ground=_ptr(g), sample_idx=_ptr(si), filter=filter,
                      stats=_ptr(out.get("stats")), proj=_ptr(out.get("boxes2d")), image_size=image_size, area_hint=_ptr(ah),
                      opts=options.codes(), frame_width=frame_width, method=meth, **src.kw)
        _enqueue(a, src.bits, table)
    if stream is not None:
        _record(stream, d.data if isinstance(d, Depth16) else d, table and depth.table, k, ii, g, si, ah, *src.keep, f.workspace, *out.values())
    return out
