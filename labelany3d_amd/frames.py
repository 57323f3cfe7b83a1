"""Images of DIFFERENT sizes in one call (include/la3d.h "images of different sizes in one call"): the frame table, the packers that
lay depth maps, label maps and mask stacks out by it (``pack_frames`` / ``pack_label_frames`` / ``pack_mask_frames``: one staging
routine, one table), the bit planes of their instances, the ``fit_instances_frames*`` fits and the checks every entry on such planes
shares (``_tabled``, ``_flat_out``, ``_on_gpu``).  ``morph``, ``rle_encode``, ``components``, ``overlap`` and ``clouds`` build on this module."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from ._device import _as_dev, _dev, _ptr, _record, _stream, _upload_many
from .batched import Depth16, _d16_block, _depth16_check, height_rule_code, padded_width, refuse_depth16
from .bits import _LOGIT_DTYPES, _crop_place, _crop_source, _crop_threshold
from .depth16 import _D16_DTYPES
from .fitcall import FramesDepth, fit_call, mask_source
from .labels import _LABEL_NUMPY, _LABEL_TORCH, _label_rows
from .segm import _rle_counts

FRAME_DTYPE = np.dtype([("depth_offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("frame_width", "<i4"), ("reserved", "<i4")])
"""One row of the frame table of a frames call: ``la3d_frame`` of include/la3d.h (24 bytes)."""


class PackedFrames(NamedTuple):
    """Depth maps of different sizes in one buffer (``pack_frames``; C-ABI ``la3d_fit_instances_frames``): ``depth`` flat float32 -
    plane p starts ``table_host["depth_offset"][p]`` floats in (a multiple of 4: 16-byte aligned), its rows ``padded_width(W_p)``
    floats apart, the columns past ``W_p`` zero -; ``table`` int32 (P, 6) on the same device: the ``la3d_frame`` rows as the kernel
    reads them; ``table_host``: the same rows as a NumPy array of ``FRAME_DTYPE``; ``H``, ``W``: the bounds of the call (largest
    rows, largest pitch); ``sizes``: the (H, W) of every image, unpadded."""
    depth: torch.Tensor
    table: torch.Tensor
    table_host: np.ndarray
    H: int
    W: int
    sizes: list


class PackedFrames16(NamedTuple):
    """16-bit depth maps of different sizes in one buffer (``pack_frames(dtype=...)``; C-ABI ``la3d_fit_instances_frames_depth16``):
    ``data`` flat ``torch.float16`` / ``torch.uint16`` - the layout of ``PackedFrames`` counted in 16-bit ELEMENTS: plane p starts
    ``table_host["depth_offset"][p]`` words in (a multiple of 4: 8-byte aligned), its rows ``padded_width(W_p)`` words apart, the
    columns past ``W_p`` zero words -; ``table`` / ``table_host`` / ``H`` / ``W`` / ``sizes`` as in ``PackedFrames``; ``scale`` /
    ``zero_is_hole``: the value rule of uint16 planes (``Depth16``; 1.0 / ignored for float16)."""
    data: torch.Tensor
    table: torch.Tensor
    table_host: np.ndarray
    H: int
    W: int
    sizes: list
    scale: float = 1.0
    zero_is_hole: bool = True


def frame_table(sizes) -> np.ndarray:
    """The frame table (``FRAME_DTYPE``) of images of the given unpadded (H, W) sizes packed back to back: pitch =
    ``padded_width(W)``, planes 16-byte aligned (every pitch is a multiple of 32 floats, so they follow each other directly)."""
    t = np.zeros(len(sizes), FRAME_DTYPE)
    off = 0
    for p, (h, w) in enumerate(sizes):
        h, w = int(h), int(w)
        if h <= 0 or w <= 0:
            raise ValueError(f"depth map {p} has an empty frame {(h, w)}")
        t[p] = (off, h, padded_width(w), w, 0)
        off += h * padded_width(w)
    return t


def table_words(table) -> np.ndarray:
    """The frame table as the int32 (P, 6) host words the kernels read (a copy; P may be 0)."""
    return np.ascontiguousarray(table).view(np.int32).reshape(len(table), 6).copy() if len(table) else np.zeros((0, 6), np.int32)


def _bounds(table):   # the bounds of a call over the table: (largest rows, largest pitch)
    return (int(table["H"].max()), int(table["W"].max())) if len(table) else (0, 0)


def _table_fields(table, sizes, dev):
    """-> (table, table_host, H, W, sizes), the fields every ``Packed*`` shares; the table goes up on the caller's current stream"""
    return (torch.as_tensor(table_words(table), device=dev), table, *_bounds(table), sizes)


def _stage_ragged(pieces, n: int, tdt, dev, pinned, wdt=None):
    """The flat buffer of a packer: ``n`` elements of ``tdt`` on ``dev``, zero wherever no piece puts a value.  A piece is ``(source,
    first element, rows, pitch, filled columns)`` in stored elements: the source, read as (rows, filled), lands at ``[first : first +
    rows * pitch]``.  The copies move ``wdt`` (default ``tdt``): the bit pattern of a dtype with few kernels, which the sources then have.
    Any CUDA source: device zeros, one device copy per piece.  Otherwise a host buffer - ``pinned[:n]`` when it has the dtype and the
    size, else a fresh one -, padding and tail zeroed, ONE upload (asynchronous when pinned); "cpu" returns the buffer."""
    wdt = tdt if wdt is None else wdt
    if any(isinstance(m, torch.Tensor) and m.is_cuda for m, *_ in pieces):
        flat = torch.zeros(n, dtype=wdt, device=dev)
        for m, first, rows, pitch, filled in pieces:
            src, dst = torch.as_tensor(m).to(device=dev, dtype=wdt), flat[first:first + rows * pitch]
            dense = pitch == filled   # (no padding: a strided source is copied straight into the destination, in its own shape)
            (dst.view(src.shape) if dense else dst.view(rows, pitch)[:, :filled]).copy_(src if dense else src.reshape(rows, filled))
        return flat.view(tdt)
    if pinned is not None and pinned.dtype == tdt and pinned.numel() >= n:
        host_t = pinned[:n]
    else:
        pinned, host_t = None, torch.empty(n, dtype=tdt)
    host, end = host_t.view(wdt).numpy(), 0
    for m, first, rows, pitch, filled in pieces:
        end = first + rows * pitch   # (the pieces follow each other)
        dst = host[first:end].reshape(rows, pitch)
        dst[:, :filled] = (m.numpy() if isinstance(m, torch.Tensor) else np.asarray(m)).reshape(rows, filled)
        dst[:, filled:] = 0
    host[end:] = 0
    return host_t if dev.type == "cpu" else host_t.view(wdt).to(dev, non_blocking=pinned is not None).view(tdt)


def _stored(m):
    """a map in its stored dtype: uint16 as int16 bit patterns (few kernels know it), bool as its bytes"""
    if isinstance(m, torch.Tensor):
        return m.view(torch.int16) if m.dtype == torch.uint16 else m.view(torch.uint8) if m.dtype == torch.bool else m
    a = np.asarray(m)
    return a.view(np.int16) if a.dtype == np.uint16 else a.view(np.uint8) if a.dtype == np.bool_ else a


def _map_pieces(maps, table, c: int = 1):
    """one map of ``c`` stored elements per pixel on every table row -> (the pieces of ``_stage_ragged``, the elements they cover)"""
    rows = [(int(r["depth_offset"]), int(r["H"]), int(r["W"]), int(r["frame_width"])) for r in table]
    return [(m, o * c, h, wp * c, w * c) for m, (o, h, wp, w) in zip(maps, rows)], sum(h * wp for _, h, wp, _ in rows) * c


def _host_or_gpu(device) -> torch.device:   # the device of a packer: "cpu" gives the layout on the host
    return torch.device(device) if device is not None and torch.device(device).type == "cpu" else _dev(device)


def _words16(m, p: int, dtype: str):
    """depth map p of a 16-bit ``pack_frames`` as its int16 bit patterns (a view where the map is contiguous): the map must already
    HAVE the 16-bit dtype - nothing is converted or rounded here"""
    tdt = _D16_DTYPES[dtype][0]
    ndt = np.float16 if dtype == "f16" else np.uint16
    if isinstance(m, torch.Tensor):
        if m.dtype != tdt:
            raise ValueError(f"depth map {p}: pack_frames(dtype={dtype!r}) takes maps of {tdt} / numpy {np.dtype(ndt).name}, not {m.dtype}")
        return m.contiguous().view(torch.int16)
    a = np.asarray(m)
    if a.dtype != ndt:
        raise ValueError(f"depth map {p}: pack_frames(dtype={dtype!r}) takes maps of numpy {np.dtype(ndt).name} / {tdt}, not {a.dtype}")
    return np.ascontiguousarray(a).view(np.int16)


def pack_frames(depth_maps, device=None, pinned=None, dtype=None, scale: float = 0.001, zero_is_hole: bool = True):
    """Depth maps of DIFFERENT sizes -> ``PackedFrames``: one flat float32 buffer on the device, each plane at its own pitch
    (``padded_width``) and 16-byte aligned offset, the padding zero, plus the device frame table ``fit_instances_frames`` takes.
    ``depth_maps``: a sequence of (H_p, W_p) arrays / tensors.  ``pinned``: a pinned float32 staging tensor of at least the packed size
    (host maps only) - the upload is then asynchronous on the current stream and the caller keeps the buffer untouched until that
    stream has passed it.  ``device="cpu"`` gives the layout on the host (no GPU needed).
    ``dtype`` "f16" / "u16": the maps already ARE 16-bit (``np.float16`` / ``np.uint16``, ``torch.float16`` / ``torch.uint16``; any
    other dtype: ValueError naming the map) and their words are copied as stored - nothing is converted or rounded - into one flat
    16-bit buffer of the same layout counted in elements: a ``PackedFrames16`` (``scale`` / ``zero_is_hole``: the value rule of uint16
    planes, see ``Depth16``; ``pinned``: a pinned staging tensor of the 16-bit dtype), fitted where it lies by ``fit_instances_frames``."""
    dev = _host_or_gpu(device)
    maps = list(depth_maps)
    if dtype is not None and dtype not in _D16_DTYPES:
        raise ValueError(f"unknown dtype: {dtype!r}. Use None (float32), 'f16' or 'u16'")
    tdt = torch.float32 if dtype is None else _D16_DTYPES[dtype][0]
    if dtype == "u16" and not (np.isfinite(np.float32(scale)) and np.float32(scale) > 0):
        raise ValueError(f"scale must be finite and > 0 (as float32), not {scale!r}")
    for p, m in enumerate(maps):
        if len(m.shape) != 2:
            raise ValueError(f"depth map {p} must be (H, W), got {tuple(m.shape)}")
    wdt = torch.float32 if dtype is None else torch.int16   # the copies move float32 (anything is converted) or the bit pattern of a 16-bit map
    if dtype is not None:
        maps = [_words16(m, p, dtype) for p, m in enumerate(maps)]
    sizes = [(int(m.shape[0]), int(m.shape[1])) for m in maps]
    table = frame_table(sizes)   # (offsets in ELEMENTS: multiples of 32, so a float32 plane is 16-byte and a 16-bit plane 8-byte aligned)
    pieces, total = _map_pieces(maps, table)
    flat = _stage_ragged(pieces, max(total, 4), tdt, dev, pinned, wdt)
    if dtype is None:
        return PackedFrames(flat, *_table_fields(table, sizes, dev))
    return PackedFrames16(flat, *_table_fields(table, sizes, dev), float(scale) if dtype == "u16" else 1.0, bool(zero_is_hole))


def pack_rle_frames(rles):
    """Run-length masks of images of different sizes -> ``(counts int32 (T,), offsets int64 (B+1,), sizes int64 (B, 2))``: ``pack_rle``
    without its one-size rule; ``sizes[n]`` = the (h, w) the annotation states, or -1 where the input does not say."""
    if isinstance(rles, tuple):
        return rles[0], rles[1], None
    counts, offsets = _rle_counts([r["counts"] for r in rles])
    sizes = np.asarray([tuple(r["size"]) for r in rles], np.int64).reshape(-1, 2)
    return counts, offsets, sizes


def _refuse_hull(method: str, who: str, instead: str) -> None:
    """The method check of the frames fits: the reference's error for an unknown method, then the refusal of the hull."""
    if _lib.method_code(method) != _lib.METHOD_PCA:
        raise ValueError(f"{who}: method='convex_hull' is not supported for frames of different sizes; group by size and use {instead}")


def _frames_depth(frames, who: str):
    """The one check of a ``frames`` argument, before any device work -> (its flat tensor, the ``FramesDepth`` of the call); where the
    buffer lives is asked afterwards (``_on_gpu``), once the caller has checked its masks."""
    refuse_depth16(frames, who)
    refuse_depth16(getattr(frames, "depth", None), who)
    if isinstance(frames, PackedFrames16):
        flat = frames.data   # (dtype, scale: the argument errors of a Depth16)
        if not isinstance(flat, torch.Tensor) or flat.dim() != 1:
            raise ValueError(f"{who}: PackedFrames16.data must be the flat tensor of pack_frames(dtype=...)")
        _depth16_check(Depth16(flat[None], frames.scale, frames.zero_is_hole))
        return flat, FramesDepth(flat, frames.table, _d16_block(flat, frames.scale, frames.zero_is_hole))
    if not isinstance(frames, PackedFrames):
        raise ValueError(f"{who}: frames must be the PackedFrames / PackedFrames16 of pack_frames")
    return frames.depth, FramesDepth(frames.depth, frames.table, None)


def _same_table(frames, bits) -> None:
    """The bit planes of a frames call were laid out for the frame table of its depth."""
    if not isinstance(bits, FrameBits):
        raise ValueError("bits must be the FrameBits of pack_label_bits_frames / pack_mask_bits_frames")
    if (bits.H, bits.W) != (frames.H, frames.W) or not np.array_equal(np.asarray(bits.table), np.asarray(frames.table_host)):
        raise ValueError("the bit planes were laid out for another frame table than the depth: pack depth and masks of the same sizes, in the same order")


def _tabled(who: str, frames, *bits) -> None:   # the ``frames`` of an entry that reads only its frame table, and the planes laid out for it
    if not isinstance(frames, _TABLED):
        raise ValueError(f"{who}: frames must be a PackedFrames / PackedFrames16 / PackedLabels / PackedMasks / FrameGrid")
    for b in bits:
        _same_table(frames, b)


def _flat_out(who, out, total, planes=None) -> None:
    """A caller's flat ``out`` (None passes) may not overlap ``planes``, the buffer the call reads, and must hold ``total`` words (None: not asked)."""
    if out is None:
        return
    flat = isinstance(out, torch.Tensor) and out.dtype == torch.int32 and out.dim() == 1
    if planes is not None and flat and out.data_ptr() < planes.data_ptr() + 4 * planes.numel() and planes.data_ptr() < out.data_ptr() + 4 * out.numel():
        raise ValueError(f"{who}: out overlaps the input planes (the call cannot work in place)")
    if total is not None and not (flat and out.is_cuda and out.is_contiguous() and out.numel() >= total and out.data_ptr() % 16 == 0):
        raise ValueError(f"{who + ': ' if who else ''}out must be a flat, 16-byte aligned int32 device tensor of at least {total} words")


def _on_gpu(flat, planes=None) -> torch.device:   # the device step of a frames entry, after every argument check
    if not flat.is_cuda or not (planes is None or planes.is_cuda):
        raise ValueError("frames and bit planes must live on the GPU (pack_frames with a GPU device)")
    if planes is not None and planes.device != flat.device:
        raise ValueError("the bit planes live on another device")
    return flat.device


def fit_instances_frames(frames, K, rles=None, polys=None, image_index=None, ground=None, sample_idx=None, filter=None, proj: bool = False,
                         area_hint=None, stream=None, method: str = "pca", _fitter=None):
    """The fit for instances of images of DIFFERENT sizes in one call (C-ABI ``la3d_fit_instances_frames``): ``frames`` is what
    ``pack_frames`` returns - a ``PackedFrames``, or a ``PackedFrames16`` (16-bit planes fitted where they lie, C-ABI
    ``la3d_fit_instances_frames_depth16``: the records of the float32 call on the up-converted planes); instance n belongs to image ``image_index[n]`` (required), whose K is ``K[image_index[n]]`` (K: (P,3,3),
    or (3,3) shared).  Exactly one of ``rles`` - a list of COCO RLE objects, each of its own image's size, or a ``(counts, offsets)``
    tuple - and ``polys`` - the tuple of ``pack_polygons`` (its H, W are ignored: every instance is clipped to its own frame) - gives
    the masks.  ``ground`` / ``sample_idx`` / ``filter`` / ``area_hint`` as in ``fit_instances_ex``; ``proj=True`` adds ``boxes2d``,
    clamped to each instance's own frame.  An instance whose image index or frame row breaks the contract of ``la3d_frame`` comes
    back with status 5 and a NaN record - decided on the device, never an exception.  ``method="convex_hull"`` is not offered in
    this form (ValueError).  Returns the dict of ``fit_instances_ex``.  The size-balanced launch order of large batches runs when
    ``area_hint`` is given."""
    _refuse_hull(method, "fit_instances_frames", "fit_instances_ex")   # (every argument error comes before any device work)
    fdepth, depth = _frames_depth(frames, "fit_instances_frames")
    if (rles is not None) + (polys is not None) != 1:
        raise ValueError("give exactly one of rles / polys")
    if image_index is None:
        raise ValueError("image_index is required: instance n belongs to frame image_index[n]")
    dev = _on_gpu(fdepth)
    if rles is not None:
        counts, offsets, sizes = pack_rle_frames(rles)
        if sizes is not None and not (isinstance(image_index, torch.Tensor) and image_index.is_cuda):
            ii_h = np.asarray(image_index.numpy() if isinstance(image_index, torch.Tensor) else image_index).reshape(-1)
            ok = (ii_h >= 0) & (ii_h < int(frames.table.shape[0]))
            if len(ii_h) == len(sizes) and ok.any():
                want = np.asarray(frames.sizes, np.int64).reshape(-1, 2)[ii_h[ok]]
                if (sizes[ok] != want).any():
                    raise ValueError("an RLE annotation's size differs from the size of its image")
        given = dict(rles=(counts, offsets, None, None))
    else:
        given = dict(polys=(polys[0], polys[1], polys[2], None, None))   # (their H, W are ignored: every instance has its own frame)
    src, ground, ii, sample_idx, area_hint = mask_source(dev, small=(ground, image_index, sample_idx, area_hint), **given)
    # (_fitter: buffers a caller keeps between calls - fit_scenes -, sized for at least this call's B and bounds)
    return fit_call(src, depth, K, dev, frames.H, frames.W, image_index=ii, ground=ground, sample_idx=sample_idx, area_hint=area_hint,
                    filter=filter, image_size=(1, 1) if proj else None, stream=stream, method=method, fitter=_fitter)


# ---- label maps and bit planes of images of different sizes (include/la3d.h "images of different sizes in one call") ----------------
class PackedLabels(NamedTuple):
    """Label maps of different sizes in one buffer (``pack_label_frames``; C-ABI ``la3d_pack_label_bits_frames``): ``data`` flat -
    ``torch.uint8`` / ``int16`` (the bit patterns of uint16 labels) / ``int32``, or ``uint8`` with 3 bytes per pixel for RGB maps -
    in the layout of ``PackedFrames`` counted in ELEMENTS (pixels for RGB): map p starts ``table_host["depth_offset"][p]`` elements
    in, its rows ``padded_width(W_p)`` elements apart, the columns past ``W_p`` zero; ``table`` / ``table_host`` / ``H`` / ``W`` /
    ``sizes`` as in ``PackedFrames`` - the table IS the one ``pack_frames`` gives for depth maps of the same sizes; ``code``: the
    element (``_lib.LABEL_*``)."""
    data: torch.Tensor
    table: torch.Tensor
    table_host: np.ndarray
    H: int
    W: int
    sizes: list
    code: int


class FrameBits(NamedTuple):
    """Bit planes of instances of images of different sizes (``pack_label_bits_frames``; C-ABI ``la3d_fit_instances_frames_bits``):
    ``bits`` flat int32 on the GPU; ``offsets`` int64 (B,) on the GPU - the plane of row b starts ``offsets[b]`` words in (a multiple of
    4) and holds the ``H_p * padded_width(W_p) / 32`` words of its image's frame -; ``image_index`` int32 (B,) and ``area`` int32 (B,)
    on the GPU as in ``LabelBits``; ``table``: the HOST frame table (``FRAME_DTYPE``) the planes were laid out for - what
    ``fit_instances_frames_bits`` compares with the table of its depth, without touching the device -; ``H``, ``W``: its bounds."""
    bits: torch.Tensor
    offsets: torch.Tensor
    image_index: torch.Tensor
    area: torch.Tensor
    table: np.ndarray
    H: int
    W: int


_LABEL_STORE = {_lib.LABEL_U8: torch.uint8, _lib.LABEL_U16: torch.int16, _lib.LABEL_I32: torch.int32, _lib.LABEL_RGB8: torch.uint8}


def pack_label_frames(label_maps, rgb: bool = False, device=None, pinned=None) -> PackedLabels:
    """Label maps of DIFFERENT sizes -> ``PackedLabels``: one flat buffer in the layout ``pack_frames`` gives depth maps of the same
    sizes (``frame_table(sizes)``: pitch ``padded_width(W)``, the padding zero), so ONE table serves ``pack_label_bits_frames`` and
    the fit.  ``label_maps``: a sequence of (H_p, W_p) arrays / tensors of ONE dtype - uint8, uint16, int16 (read as uint16) or int32 -
    or, with ``rgb=True``, of (H_p, W_p, 3) uint8 maps (a COCO panoptic PNG as it decodes).  ``pinned``: a pinned staging tensor of
    the stored dtype and at least the packed size (host maps only; the upload is then asynchronous on the current stream).
    ``device="cpu"`` gives the layout on the host (no GPU needed)."""
    dev = _host_or_gpu(device)
    maps = list(label_maps)
    code, c = None, 3 if rgb else 1
    for p, m in enumerate(maps):
        one = _LABEL_TORCH.get(m.dtype) if isinstance(m, torch.Tensor) else _LABEL_NUMPY.get(np.asarray(m).dtype)
        if one is None:
            raise ValueError(f"label map {p} must be uint8, uint16, int16 (read as uint16) or int32, not {getattr(m, 'dtype', type(m).__name__)}")
        if rgb and (one != _lib.LABEL_U8 or len(m.shape) != 3 or m.shape[-1] != 3):
            raise ValueError(f"label map {p}: rgb=True takes (H, W, 3) uint8 maps, not {tuple(m.shape)} {m.dtype}")
        if not rgb and len(m.shape) != 2:
            raise ValueError(f"label map {p} must be (H, W), got {tuple(m.shape)}")
        if code is not None and one != code:
            raise ValueError(f"label map {p} has another dtype than label map 0: pack maps of one dtype")
        code = one
    code = _lib.LABEL_RGB8 if rgb else (code if code is not None else _lib.LABEL_U8)
    tdt = _LABEL_STORE[code]
    maps = [_stored(m) for m in maps]
    sizes = [(int(m.shape[0]), int(m.shape[1])) for m in maps]
    table = frame_table(sizes)
    pieces, total = _map_pieces(maps, table, c)
    flat = _stage_ragged(pieces, max(total, 16 * c), tdt, dev, pinned)
    return PackedLabels(flat, *_table_fields(table, sizes, dev), code)


def frame_bits_offsets(table, image_index):
    """The layout ``pack_label_bits_frames`` gives the planes of host ids: -> (offsets int64 (B,), total words).  Row b gets the
    ``H * W / 32`` words of the frame row ``table[image_index[b]]`` (W: the pitch, a multiple of 32); the planes follow each other
    in row order, each start rounded up to a multiple of 4 words (16 bytes)."""
    ii = np.asarray(image_index, np.int64).reshape(-1)
    words = (table["H"].astype(np.int64) * table["W"].astype(np.int64) // 32)[ii] if len(ii) else np.zeros(0, np.int64)
    step = (words + 3) // 4 * 4
    offsets = np.zeros(len(ii), np.int64)
    np.cumsum(step[:-1], out=offsets[1:])
    return offsets, int(step.sum())


def _table_device(frames, out, total: int):   # a packer that reads only the frame table -> (the table's device, P), ``out`` checked there
    if not (isinstance(frames.table, torch.Tensor) and frames.table.is_cuda):
        raise ValueError("the frame table must live on the GPU (pack_frames with a GPU device)")
    if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == frames.table.device):
        raise ValueError("out must be a flat int32 tensor on the device of the frame table")
    _flat_out(None, out, total)   # (before anything is uploaded)
    return frames.table.device, len(frames.sizes)


def _bits_buffers(out, total: int, B: int, dev):
    """The outputs of a frames bit packer -> (the ``total`` plane words: ``out`` where it is given and fits, the B areas)."""
    _flat_out(None, out, total)
    return torch.empty(max(total, 4), dtype=torch.int32, device=dev) if out is None else out, torch.empty(B, dtype=torch.int32, device=dev)


def pack_label_bits_frames(labels: PackedLabels, ids, stream=None, out=None) -> FrameBits:
    """``pack_label_bits`` for label maps of different sizes (C-ABI ``la3d_pack_label_bits_frames``): one launch reads every map once
    and writes, per (image, id) row, the bit plane ``labels[image] == id`` of the image's OWN frame - ``H_p * padded_width(W_p) / 32``
    words, the bits of the padding columns zero whatever id is asked (id 0 of a zero-padded map marks image pixels only).
    ``labels``: a resident ``PackedLabels``; ``ids`` as in ``pack_label_bits``.  Host ids: the planes follow each other, each start
    rounded up to 4 words (``frame_bits_offsets``), and offsets, ids and image indices go up in ONE copy.  Device ids: no
    synchronisation - the sizes of the rows are then unknown here, so the planes lie a uniform stride apart, the words of the bounds'
    frame rounded up to 4.  ``out``: a flat int32 device tensor of at least that many words to fill (only the words of each plane are
    written).  Returns ``FrameBits``; an id that is absent or outside the dtype's range gives an all-zero plane of area 0."""
    if not isinstance(labels, PackedLabels):
        raise ValueError("labels must be the PackedLabels of pack_label_frames")
    P = len(labels.sizes)
    lab, off, ii, B = _label_rows(ids, P)
    if not labels.data.is_cuda:
        raise ValueError("the label maps must live on the GPU (pack_label_frames with a GPU device)")
    dev = labels.data.device
    with torch.cuda.device(dev):
        if ii is not None:
            offs_h, total = frame_bits_offsets(labels.table_host, ii)
            lab, off, ii, offs = _upload_many([(lab, torch.int32), (off, torch.int32), (ii, torch.int32), (offs_h, torch.int64)], dev)
        else:
            lab, off = _as_dev(lab, torch.int32, dev), _as_dev(off, torch.int32, dev)
            ii = torch.searchsorted(off[1:].contiguous(), torch.arange(B, dtype=torch.int32, device=dev), right=True).to(torch.int32)
            stride = (labels.H * labels.W // 32 + 3) // 4 * 4
            offs, total = torch.arange(B, dtype=torch.int64, device=dev) * stride, B * stride
        o, area = _bits_buffers(out, total, B, dev)
        check(lib.la3d_pack_label_bits_frames(_ptr(labels.data), labels.code, _ptr(labels.table), P, labels.H, labels.W, _ptr(off), _ptr(lab), B,
                                              _ptr(o), _ptr(offs), _ptr(area), _stream(stream)), "la3d_pack_label_bits_frames")
    _record(stream, labels.data, labels.table, lab, off, ii, offs, o, area)
    return FrameBits(o, offs, ii, area, labels.table_host, labels.H, labels.W)


def fit_instances_frames_bits(frames, bits: FrameBits, K, image_index=None, ground=None, sample_idx=None, filter=None, proj: bool = False,
                              area_hint=None, height_rule: str = "rows", stream=None, method: str = "pca", _fitter=None):
    """``fit_instances_frames`` with the masks given as bit planes, one per instance, each of its own image's frame (C-ABI
    ``la3d_fit_instances_frames_bits``): what ``pack_label_bits_frames`` makes of the label maps of a panoptic dataset, or
    ``pack_mask_bits_frames`` of the per-image mask / logit stacks of an instance-segmentation network.  ``frames``: a
    ``PackedFrames`` or ``PackedFrames16`` laid out by the SAME frame table as the planes (``bits.table``; a mismatch is a ValueError
    before any device work); ``image_index`` defaults to ``bits.image_index``; ``ground`` / ``sample_idx`` / ``filter`` / ``proj`` /
    ``area_hint`` as in ``fit_instances_frames``, ``height_rule`` as in ``fit_instances_bits``.  An instance whose image index, frame
    row or plane offset breaks the contract comes back with status 5 and a NaN record - decided on the device, never an exception.
    ``method="convex_hull"`` is not offered for frames of different sizes (ValueError).  Returns the dict of ``fit_instances_frames``."""
    _refuse_hull(method, "fit_instances_frames_bits", "fit_instances_bits")   # (every argument error comes before any device work)
    flags = height_rule_code(height_rule)
    fdepth, depth = _frames_depth(frames, "fit_instances_frames_bits")
    _same_table(frames, bits)
    dev = _on_gpu(fdepth, bits.bits)
    src, ground, ii, sample_idx, area_hint = mask_source(dev, frame_bits=(bits, flags), small=(
        ground, bits.image_index if image_index is None else image_index, sample_idx, area_hint))
    return fit_call(src, depth, K, dev, frames.H, frames.W, image_index=ii, ground=ground, sample_idx=sample_idx, area_hint=area_hint,
                    filter=filter, image_size=(1, 1) if proj else None, stream=stream, method=method, fitter=_fitter)


def _device_of(frames):   # where the buffer of a (not yet checked) frames argument lives: what a pack-then-fit call packs its masks for
    return getattr(getattr(frames, "data" if isinstance(frames, PackedFrames16) else "depth", None), "device", None)


def _fit_packed(frames, fb: FrameBits, K, **kw):   # the tail of a pack-then-fit call: the planes' exact areas as area_hint, "bits" added
    out = fit_instances_frames_bits(frames, fb, K, area_hint=fb.area, **kw)
    out["bits"] = fb
    return out


def fit_instances_frames_labels(frames, label_maps, ids, K, image_index=None, ground=None, sample_idx=None, filter=None, proj: bool = False,
                                height_rule: str = "rows", stream=None, method: str = "pca", rgb: bool = False):
    """The depth + mask fit of every listed instance of label maps of DIFFERENT sizes in one call: ``pack_label_frames`` (skipped for a
    ``PackedLabels``), ``pack_label_bits_frames`` (one pass over the labels), then ``fit_instances_frames_bits`` with the rows'
    ``image_index`` and their exact areas as ``area_hint``.  ``frames``: the ``PackedFrames`` / ``PackedFrames16`` of the depth maps of
    the same images in the same order; ``label_maps`` / ``rgb`` as in ``pack_label_frames``; ``ids`` as in ``pack_label_bits``; the
    other arguments as in ``fit_instances_frames_bits``, per (image, id) row in ``ids`` order.  Returns its dict plus ``"bits"``: the
    ``FrameBits``.  With resident ``PackedLabels`` and device ids nothing synchronises and the call can be captured into a graph."""
    _refuse_hull(method, "fit_instances_frames_labels", "fit_instances_labels")
    height_rule_code(height_rule)
    pl = label_maps if isinstance(label_maps, PackedLabels) else pack_label_frames(label_maps, rgb=rgb, device=_device_of(frames))
    fb = pack_label_bits_frames(pl, ids, stream=stream)
    return _fit_packed(frames, fb, K, image_index=image_index, ground=ground, sample_idx=sample_idx, filter=filter, proj=proj,
                       height_rule=height_rule, stream=stream, method=method)


# ---- network masks and logits of images of different sizes (include/la3d.h: la3d_pack_mask_bits_frames / la3d_pack_logits_bits_frames) --
MASKS_U8 = -1
"""``PackedMasks.kind`` of uint8 / boolean masks; logits carry their ``_lib.DTYPE_*`` code."""
_MASK_TORCH = {torch.bool: MASKS_U8, torch.uint8: MASKS_U8, **_LOGIT_DTYPES}
_MASK_NUMPY = {np.dtype(np.bool_): MASKS_U8, np.dtype(np.uint8): MASKS_U8, np.dtype(np.float32): _lib.DTYPE_F32, np.dtype(np.float16): _lib.DTYPE_F16}
_MASK_STORE = {MASKS_U8: torch.uint8, _lib.DTYPE_F32: torch.float32, _lib.DTYPE_F16: torch.float16, _lib.DTYPE_BF16: torch.bfloat16}


class PackedMasks(NamedTuple):
    """Per-image stacks of masks or logits of different sizes behind one base pointer (``pack_mask_frames``; C-ABI
    ``la3d_pack_mask_bits_frames`` / ``la3d_pack_logits_bits_frames``): ``data`` flat ``torch.uint8`` / ``float32`` / ``float16`` /
    ``bfloat16`` - the plane of row n starts ``offsets[n]`` ELEMENTS (int64 (B,)) behind ``data``'s first element and has the
    ``(H_p, W_p)`` of image ``image_index[n]`` (int32 (B,)), its rows ``pitch[n]`` elements apart (int32 (B,); None: ``W_p`` apart -
    dense planes) -; ``table`` / ``table_host`` / ``H`` / ``W`` / ``sizes`` as in ``PackedFrames`` - the table IS the one
    ``pack_frames`` gives depth maps of the same sizes; ``kind``: ``MASKS_U8`` or the logits' ``_lib.DTYPE_*`` code;
    ``bits_offsets`` int64 (B,) on the device of ``data`` / ``bits_words``: the layout ``frame_bits_offsets`` gives the bit planes of
    these rows (resident, so that ``pack_mask_bits_frames`` uploads nothing; None / 0: computed there); ``sources``: the tensors
    ``data`` aliases (a zero-copy pack), kept alive with the result."""
    data: torch.Tensor
    offsets: torch.Tensor
    pitch: Optional[torch.Tensor]
    image_index: torch.Tensor
    table: torch.Tensor
    table_host: np.ndarray
    H: int
    W: int
    sizes: list
    kind: int
    bits_offsets: Optional[torch.Tensor] = None
    bits_words: int = 0
    sources: tuple = ()


def _mask_stacks(stacks):
    """the argument errors of per-image mask stacks that need no device -> (stacks, kind, sizes, counts)"""
    stacks = list(stacks)
    kind = None
    for p, m in enumerate(stacks):
        dt = m.dtype if isinstance(m, torch.Tensor) else np.asarray(m).dtype
        one = _MASK_TORCH.get(dt) if isinstance(m, torch.Tensor) else _MASK_NUMPY.get(dt)
        if one is None:
            raise ValueError(f"mask stack {p} (image {p}) must be bool, uint8, float32, float16 or bfloat16, not {dt}")
        if len(m.shape) != 3:
            raise ValueError(f"mask stack {p} (image {p}) must be (N, H, W), got {tuple(m.shape)}")
        if kind is not None and one != kind:
            raise ValueError(f"mask stack {p} (image {p}) has another dtype than mask stack 0: pack stacks of one dtype")
        kind = one
        if int(m.shape[1]) <= 0 or int(m.shape[2]) <= 0:
            raise ValueError(f"mask stack {p} (image {p}) has an empty frame {(int(m.shape[1]), int(m.shape[2]))}")
    sizes = [(int(m.shape[1]), int(m.shape[2])) for m in stacks]
    counts = [int(m.shape[0]) for m in stacks]
    return stacks, (MASKS_U8 if kind is None else kind), sizes, counts


def _mask_in_place(m, dev) -> bool:
    """a device stack the packer can read where it lies: adjacent pixels, rows at least a frame's width apart"""
    if not (isinstance(m, torch.Tensor) and m.is_cuda and m.device == dev):
        return False
    n, h, w = m.shape
    return (w == 1 or m.stride(2) == 1) and (h == 1 or m.stride(1) >= w) and m.stride(1) < 2 ** 31


def pack_mask_frames(stacks, device=None, pinned=None) -> PackedMasks:
    """The outputs of an instance-segmentation network for images of DIFFERENT sizes -> ``PackedMasks``.  ``stacks``: a sequence over
    IMAGES of (N_p, H_p, W_p) arrays / tensors (N_p may be 0), all of ONE dtype out of bool / uint8 (masks: non-zero = inside) and
    float32 / float16 / bfloat16 (logits, thresholded by ``pack_mask_bits_frames``); row n of the result is the n-th plane in image
    order.  The table is ``frame_table(sizes)`` - the one ``pack_frames`` gives depth maps of the same sizes, so ONE table serves the
    packer and the fit.
    Host stacks are laid back to back, dense - no padding of the rows -, into one buffer and uploaded in one copy (``pinned``: a pinned
    staging tensor of the stored dtype and at least the packed size; the upload is then asynchronous on the current stream).
    DEVICE stacks whose planes have adjacent pixels (``stride(2) == 1``, ``stride(1) >= W_p``) are NOT copied: ``data`` is a flat view
    based at the lowest ``data_ptr()`` among them, ``offsets`` the element distances from there and ``pitch`` given where any
    ``stride(1) != W_p`` - a network's outputs read where they lie, the top-left crop of a padded canvas included; the result keeps
    the tensors alive (``sources``).  Anything else is made dense first.  ``device="cpu"`` gives the dense layout on the host (no GPU
    needed).  ValueError, naming the image: mixed dtypes, a stack that is not 3-D, an empty frame."""
    stacks, kind, sizes, counts = _mask_stacks(stacks)
    dev = _host_or_gpu(device)
    tdt = _MASK_STORE[kind]
    es = torch.empty(0, dtype=tdt).element_size()
    table = frame_table(sizes)
    P, B = len(stacks), sum(counts)
    ii = np.repeat(np.arange(P, dtype=np.int32), counts)
    pitch, sources = None, ()
    live = [m for m, c in zip(stacks, counts) if c]
    if dev.type == "cuda" and live and all(_mask_in_place(m, dev) for m in live):
        live = [_stored(m) for m in live]
        low = min(live, key=lambda m: m.data_ptr())
        base = low.data_ptr()
        data = low.as_strided((low.untyped_storage().nbytes() // es - low.storage_offset(),), (1,))
        offs, pit = [], []
        for m, c, (h, w) in zip(stacks, counts, sizes):
            if c:
                first = (m.data_ptr() - base) // es
                offs.append(first + np.arange(c, dtype=np.int64) * (m.stride(0) if c > 1 else 0))
                pit.append(np.full(c, m.stride(1) if h > 1 else w, np.int32))
        offsets = np.concatenate(offs)
        pit = np.concatenate(pit)
        if (pit != np.asarray(sizes, np.int64).reshape(-1, 2)[ii, 1]).any():
            pitch = pit
        sources = tuple(live)
    else:
        words = np.asarray([h * w for h, w in sizes], np.int64)[ii] if B else np.zeros(0, np.int64)
        offsets = np.zeros(B, np.int64)
        np.cumsum(words[:-1], out=offsets[1:])
        starts = np.concatenate([[0], np.cumsum([c * h * w for c, (h, w) in zip(counts, sizes)])]).astype(np.int64)
        wdt = torch.int16 if tdt == torch.bfloat16 else tdt   # (NumPy has no bfloat16: the copies move its bit patterns)
        pieces = [(_stored(m) if wdt == tdt else m.view(wdt), int(o), c * h, w, w) for m, o, c, (h, w) in zip(stacks, starts, counts, sizes) if c]
        data = _stage_ragged(pieces, max(int(words.sum()), 16), tdt, dev, pinned, wdt)
    boffs, bwords = frame_bits_offsets(table, ii)
    small = [(offsets, torch.int64), (boffs, torch.int64), (ii, torch.int32), (table_words(table), torch.int32), (pitch, torch.int32)]
    if dev.type == "cpu":
        offs_t, boffs_t, ii_t, tab, pitch_t = [None if a is None else torch.as_tensor(np.ascontiguousarray(a)) for a, _ in small]
    else:
        with torch.cuda.device(dev):
            offs_t, boffs_t, ii_t, tab, pitch_t = _upload_many(small, dev)
    return PackedMasks(data, offs_t, pitch_t, ii_t, tab, table, *_bounds(table), sizes, kind, boffs_t, bwords, sources)


def pack_mask_bits_frames(masks, threshold: float = 0.0, stream=None, out=None) -> FrameBits:
    """``pack_mask_bits`` / ``pack_logits_bits`` for the stacks of images of different sizes (C-ABI ``la3d_pack_mask_bits_frames`` /
    ``la3d_pack_logits_bits_frames``): ONE launch reads every plane once, where it lies, and writes per row the bit plane of its
    image's OWN frame - ``H_p * padded_width(W_p) / 32`` words, the bits of the padding columns zero - laid out by
    ``frame_bits_offsets(table_host, image_index)``.  ``masks``: a ``PackedMasks``, or a sequence that goes through
    ``pack_mask_frames``; ``threshold``: logits only (bit = x > threshold in float32; NaN gives 0); ``out``: as in
    ``pack_label_bits_frames``.  With a resident ``PackedMasks`` nothing is uploaded and nothing synchronises.  Returns ``FrameBits``."""
    pm = masks if isinstance(masks, PackedMasks) else pack_mask_frames(masks)
    if pm.kind not in _MASK_STORE or pm.data.dtype != _MASK_STORE[pm.kind]:
        raise ValueError(f"PackedMasks.kind {pm.kind!r} does not name the dtype of its data ({pm.data.dtype})")
    if not pm.data.is_cuda:
        raise ValueError("the masks must live on the GPU (pack_mask_frames with a GPU device)")
    dev = pm.data.device
    P, B = len(pm.sizes), int(pm.offsets.numel())
    with torch.cuda.device(dev):
        if pm.bits_offsets is None:
            offs_h, total = frame_bits_offsets(pm.table_host, pm.image_index.cpu().numpy())
            offs = _as_dev(offs_h, torch.int64, dev)
        else:
            offs, total = pm.bits_offsets, int(pm.bits_words)
        o, area = _bits_buffers(out, total, B, dev)
        tail = (_ptr(pm.table), P, pm.H, pm.W, _ptr(pm.image_index), _ptr(pm.offsets), _ptr(pm.pitch), B, _ptr(o), _ptr(offs), _ptr(area),
                _stream(stream))
        if pm.kind == MASKS_U8:
            check(lib.la3d_pack_mask_bits_frames(_ptr(pm.data), *tail), "la3d_pack_mask_bits_frames")
        else:
            check(lib.la3d_pack_logits_bits_frames(_ptr(pm.data), pm.kind, float(threshold), *tail), "la3d_pack_logits_bits_frames")
    _record(stream, pm.data, pm.table, pm.image_index, pm.offsets, pm.pitch, offs, o, area, *pm.sources)
    return FrameBits(o, offs, pm.image_index, area, pm.table_host, pm.H, pm.W)


# ---- annotations of images of different sizes as bit planes (include/la3d.h "annotations as bit planes") ---------------------------
def _annotation_rows(who, frames, B: int, image_index, sizes=None):
    """The argument errors of ``pack_rle_bits_frames`` / ``pack_poly_bits_frames``, before any device work -> (host image indices or
    None for a device ``image_index``, the host plane offsets or None, the words of all planes)."""
    if not isinstance(frames, (PackedFrames, PackedFrames16)):
        raise ValueError(f"{who}: frames must be the PackedFrames / PackedFrames16 of pack_frames")
    if image_index is None:
        raise ValueError(f"{who}: image_index is required: instance n belongs to frame image_index[n]")
    P = len(frames.sizes)
    stride = (frames.H * frames.W // 32 + 3) // 4 * 4   # the words of the bounds' frame, rounded up to 16 bytes
    if isinstance(image_index, torch.Tensor) and image_index.is_cuda:
        if image_index.dim() != 1 or image_index.numel() != B:
            raise ValueError(f"{who}: image_index must hold one image per annotation ({B}), got {tuple(image_index.shape)}")
        return None, None, B * stride
    ii = np.asarray(image_index.numpy() if isinstance(image_index, torch.Tensor) else image_index).reshape(-1)
    if len(ii) != B:
        raise ValueError(f"{who}: image_index must hold one image per annotation ({B}), got {len(ii)}")
    if B and not np.issubdtype(ii.dtype, np.integer):
        raise ValueError(f"{who}: image_index must be integers")
    ii = ii.astype(np.int64)
    if B and (int(ii.min()) < 0 or int(ii.max()) >= P):
        raise ValueError(f"{who}: image_index must lie in [0, {P})")
    if sizes is not None and B and (sizes != np.asarray(frames.sizes, np.int64).reshape(-1, 2)[ii]).any():
        raise ValueError("an RLE annotation's size differs from the size of its image")
    offs, total = frame_bits_offsets(frames.table_host, ii)
    return ii, offs, total


def _pack_annotation_bits_frames(entry, name, frames, arrays, B, image_index, ii_h, offs_h, total, stream, out) -> FrameBits:
    """The device step the two annotation packers share: the small arrays up in one copy, the planes' buffers, the call."""
    dev, P = _table_device(frames, out, total)
    with torch.cuda.device(dev):
        resident = all(isinstance(a, torch.Tensor) and a.is_cuda for a, _ in arrays)   # annotation arrays that are on a GPU already
        if resident:
            ann = [_as_dev(a, dt, dev) for a, dt in arrays]
            ii, offs = (None, None) if ii_h is None else _upload_many([(ii_h, torch.int32), (offs_h, torch.int64)], dev)
        elif ii_h is not None:
            *ann, ii, offs = _upload_many(arrays + [(ii_h, torch.int32), (offs_h, torch.int64)], dev)
        else:
            ann = _upload_many(arrays, dev)
        if ii_h is None:
            ii = _as_dev(image_index, torch.int32, dev)
            offs = torch.arange(B, dtype=torch.int64, device=dev) * (total // B if B else 0)
        o, area = _bits_buffers(out, total, B, dev)
        check(entry(*[_ptr(a) for a in ann], _ptr(frames.table), P, frames.H, frames.W, _ptr(ii), B, _ptr(o), _ptr(offs), _ptr(area),
                    _stream(stream)), name)
    _record(stream, frames.table, *ann, ii, offs, o, area)
    return FrameBits(o, offs, ii, area, frames.table_host, frames.H, frames.W)


def pack_rle_bits_frames(frames, rles, image_index, stream=None, out=None) -> FrameBits:
    """COCO run lengths of images of DIFFERENT sizes -> ``FrameBits`` (C-ABI ``la3d_pack_rle_bits_frames``): one launch decodes every
    annotation into the bit plane of its image's OWN frame - ``H_p * padded_width(W_p) / 32`` words, the bits of the padding columns
    zero -, what ``instance_points_frames`` and ``fit_instances_frames_bits`` take.  ``frames``: a ``PackedFrames`` /
    ``PackedFrames16`` (only its table, bounds and sizes are used); ``rles``: a list of COCO RLE objects, each of its own image's size
    (another stated size: ValueError), or a ``(counts, offsets)`` tuple; instance n belongs to image ``image_index[n]``.  Host
    ``image_index``: the planes are laid out by ``frame_bits_offsets`` and the small arrays go up in ONE copy.  Device
    ``image_index``: no synchronisation - the planes lie a uniform stride apart, the words of the bounds' frame rounded up to 4, and the
    stated sizes are NOT compared with the images' (which image a row belongs to is unknown here without reading the index back): the
    runs are then decoded over the image's own frame, whatever the annotation states.
    ``out``: as in ``pack_label_bits_frames``.  An instance whose image index or frame row breaks the contract gets no plane and
    area 0 - decided on the device."""
    counts, offsets, sizes = pack_rle_frames(rles)
    B = len(offsets) - 1
    ii_h, offs_h, total = _annotation_rows("pack_rle_bits_frames", frames, B, image_index, sizes)
    return _pack_annotation_bits_frames(lib.la3d_pack_rle_bits_frames, "la3d_pack_rle_bits_frames", frames,
                                        [(counts, torch.int32), (offsets, torch.int64)], B, image_index, ii_h, offs_h, total, stream, out)


def pack_poly_bits_frames(frames, polys, image_index, stream=None, out=None) -> FrameBits:
    """Polygon parts of images of DIFFERENT sizes -> ``FrameBits`` (C-ABI ``la3d_pack_poly_bits_frames``): ``polys`` is the tuple of
    ``pack_polygons`` (its H, W are ignored: every instance is clipped to its own frame).  Other arguments and the result as
    ``pack_rle_bits_frames``."""
    if not (isinstance(polys, tuple) and len(polys) == 5):
        raise ValueError("polys must be the (xy, ring_offsets, inst_rings, H, W) tuple of pack_polygons")
    B = len(polys[2]) - 1
    ii_h, offs_h, total = _annotation_rows("pack_poly_bits_frames", frames, B, image_index)
    return _pack_annotation_bits_frames(lib.la3d_pack_poly_bits_frames, "la3d_pack_poly_bits_frames", frames,
                                        [(polys[0], torch.int32), (polys[1], torch.int64), (polys[2], torch.int64)], B, image_index, ii_h,
                                        offs_h, total, stream, out)


def pack_crop_bits_frames(frames, crops, params, image_index, threshold=None, stream=None, out=None) -> FrameBits:
    """Crop-space masks of images of DIFFERENT sizes -> ``FrameBits`` (C-ABI ``la3d_pack_crop_bits_frames``): ``pack_crop_bits`` with
    every crop restored into the bit plane of its image's OWN frame - ``H_p * padded_width(W_p) / 32`` words, the bits of the padding
    columns zero.  ``crops`` / ``params`` / ``threshold`` as in ``pack_crop_bits``; ``frames`` / ``image_index`` / ``out`` and the
    result as in ``pack_rle_bits_frames`` (host ``image_index``: planes laid out by ``frame_bits_offsets``; device ``image_index``: no
    synchronisation, a uniform stride).  An instance whose image index or frame row breaks the contract gets no plane and area 0 -
    decided on the device."""
    who = "pack_crop_bits_frames"
    B = int(crops.shape[0]) if hasattr(crops, "shape") else len(crops)
    ii_h, offs_h, total = _annotation_rows(who, frames, B, image_index)
    dev, P = _table_device(frames, out, total)
    with torch.cuda.device(dev):
        v, sb, sr, sp, S, B, default = _crop_source(who, crops, dev)
        thr = _crop_threshold(who, threshold, default)
        place = _crop_place(who, params, S, B, dev)
        if ii_h is not None:
            ii, offs = _upload_many([(ii_h, torch.int32), (offs_h, torch.int64)], dev)
        else:
            ii = _as_dev(image_index, torch.int32, dev)
            offs = torch.arange(B, dtype=torch.int64, device=dev) * (total // B if B else 0)
        o, area = _bits_buffers(out, total, B, dev)
        check(lib.la3d_pack_crop_bits_frames(v.data_ptr(), sb, sr, sp, S, thr, _ptr(place), _ptr(frames.table), P, frames.H, frames.W, _ptr(ii), B,
                                             _ptr(o), _ptr(offs), _ptr(area), _stream(stream)), "la3d_pack_crop_bits_frames")
    _record(stream, frames.table, v, place, ii, offs, o, area)
    return FrameBits(o, offs, ii, area, frames.table_host, frames.H, frames.W)


class FrameGrid(NamedTuple):
    """A frame table without data (``scaled_frames``): the ``table`` / ``table_host`` / ``H`` / ``W`` / ``sizes`` fields every
    ``Packed*`` has - what the entries that use only the table of their ``frames`` argument take in its place."""
    table: torch.Tensor
    table_host: np.ndarray
    H: int
    W: int
    sizes: list


_TABLED = (PackedFrames, PackedFrames16, PackedLabels, PackedMasks, FrameGrid)   # what an entry that reads only the frame table takes


def _upscale_arg(who: str, upscale) -> None:   # the upscale of an opening (morph) and of the frame table of its result
    if isinstance(upscale, bool) or not isinstance(upscale, (int, np.integer)) or int(upscale) not in (1, 2, 4):
        raise ValueError(f"{who}: upscale must be 1, 2 or 4 (factors whose nearest-neighbour rule is u // s under every convention), not {upscale!r}")


def _scaled_sizes(frames, s: int) -> list:
    return [(s * int(h), s * int(w)) for h, w in frames.sizes]


def _scaled_table(table, s: int) -> np.ndarray:
    """``frame_table`` of the sizes ``(s * H, s * frame_width)`` of a host frame table, without a Python loop over the images"""
    t = np.zeros(len(table), FRAME_DTYPE)
    t["H"], t["frame_width"] = table["H"] * s, table["frame_width"] * s
    t["W"] = (t["frame_width"] + 31) // 32 * 32
    np.cumsum((t["H"].astype(np.int64) * t["W"])[:-1], out=t["depth_offset"][1:])
    return t


def scaled_frames(frames, upscale: int, device=None) -> FrameGrid:
    """The frame table of the images of ``frames`` (a ``Packed*`` or a ``FrameGrid``) upscaled by ``upscale``: ``frame_table`` of the
    sizes ``(s * h, s * w)`` with its bounds - the layout of the planes ``open_bits_frames(..., upscale=s)`` returns, for
    ``rle_encode_bits_frames`` and ``bits_rects_frames`` on them.  One small upload, to ``device`` (default: where the table of
    ``frames`` lives; "cpu" gives the table on the host)."""
    _tabled("scaled_frames", frames)
    _upscale_arg("scaled_frames", upscale)
    dev = frames.table.device if device is None else _host_or_gpu(device)
    sizes = _scaled_sizes(frames, int(upscale))
    return FrameGrid(*_table_fields(frame_table(sizes), sizes, dev))


def fit_instances_frames_masks(frames, masks, K, threshold: float = 0.0, image_index=None, ground=None, sample_idx=None, filter=None,
                               proj: bool = False, height_rule: str = "rows", stream=None, method: str = "pca"):
    """The depth + mask fit of the per-image mask / logit stacks of an instance-segmentation network, images of DIFFERENT sizes, in
    one call: ``pack_mask_frames`` (skipped for a ``PackedMasks``), ``pack_mask_bits_frames`` (one launch over the planes where they
    lie), then ``fit_instances_frames_bits`` with the rows' ``image_index`` and their exact areas as ``area_hint``.  ``frames``: the
    ``PackedFrames`` / ``PackedFrames16`` of the depth maps of the same images in the same order (another ``(H_p, W_p)`` than the
    masks': ValueError before any device work); ``threshold``: logits only; the other arguments as in ``fit_instances_frames_bits``,
    per plane in image order.  Returns its dict plus ``"bits"``: the ``FrameBits``.  With a resident ``PackedMasks`` nothing
    synchronises and the call can be captured into a graph."""
    _refuse_hull(method, "fit_instances_frames_masks", "fit_instances_bits")
    height_rule_code(height_rule)
    if isinstance(masks, PackedMasks):
        sizes = masks.sizes
    else:
        masks, _, sizes, _ = _mask_stacks(masks)
    if [tuple(s) for s in sizes] != [tuple(s) for s in getattr(frames, "sizes", ())]:
        raise ValueError("the masks have another (H, W) per image than the depth: give one stack per depth map, each of its image's size, in the same order")
    pm = masks if isinstance(masks, PackedMasks) else pack_mask_frames(masks, device=_device_of(frames))
    fb = pack_mask_bits_frames(pm, threshold=threshold, stream=stream)
    return _fit_packed(frames, fb, K, image_index=image_index, ground=ground, sample_idx=sample_idx, filter=filter, proj=proj,
                       height_rule=height_rule, stream=stream, method=method)
