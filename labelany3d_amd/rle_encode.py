"""Bit planes as run lengths (include/la3d.h): COCO run lengths of ``MaskBits`` and of ``FrameBits``, and the JSON objects made of them."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._device import _as_dev, _record, _stream
from ._lib import check, lib
from .batched import _bits_stride
from .bits import MaskBits, _mask_bits, pack_mask_bits
from .frames import FrameBits, _on_gpu, _tabled


class RleRuns(NamedTuple):
    """What ``rle_encode_bits`` / ``rle_encode`` return: the COCO run lengths of B masks of one frame size, on the GPU - ``counts``
    int32 (capacity,): the run list of instance n is ``counts[offsets[n]:offsets[n+1]]``, column-major over (H, W), zeros first;
    ``offsets`` int64 (B+1,); ``H``, ``W``: the IMAGE (W = its columns, never a padded pitch).  It is the 4-tuple ``pack_rle`` passes
    through: ``fit_instances_rle``, ``fit_instances_ex(rles=...)``, ``pack_rle_bits``, ``rle_decode`` and ``mask_stats_rle`` take it as
    it is."""
    counts: torch.Tensor
    offsets: torch.Tensor
    H: int
    W: int


def rle_to_string(counts) -> str:
    """Run lengths -> COCO compressed RLE string (pycocotools rleToString), via the library's host helper: the inverse of
    ``rle_from_string``."""
    c = np.ascontiguousarray(counts.cpu().numpy() if isinstance(counts, torch.Tensor) else counts, dtype=np.int32).reshape(-1)
    cap = 7 * len(c) + 1   # (a count or a difference of two has at most 33 bits and a sign: seven 5-bit groups)
    buf = C.create_string_buffer(cap)
    n = lib.la3d_rle_to_string_host(c.ctypes.data, len(c), buf, cap)
    if n < 0:
        raise ValueError("la3d_rle_to_string_host refused the counts")
    return buf.raw[:n].decode("ascii")


def _rle_capacity(who: str, capacity) -> None:
    if capacity is not None and (not isinstance(capacity, (int, np.integer)) or isinstance(capacity, bool) or int(capacity) < 0):
        raise ValueError(f"{who}: capacity must be None or an int >= 0, not {capacity!r}")


def _rle_encode_run(a: _lib.RleEncodeArgs, B: int, dev, capacity, stream, keep):
    """Both stages of one call.  ``a``: the block with every input set -> (counts, offsets, status)."""
    with torch.cuda.device(dev):
        a.stream = _stream(stream)
        runs = torch.empty(max(B, 1), dtype=torch.int32, device=dev)
        offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
        ws = torch.empty(max(int(lib.la3d_rle_encode_workspace_bytes(B, a.H, a.W)) // 8, 1), dtype=torch.int64, device=dev)
        a.runs, a.offsets, a.workspace = runs.data_ptr(), offsets.data_ptr(), ws.data_ptr()
        check(lib.la3d_rle_encode_offsets(C.byref(a)), "la3d_rle_encode_offsets")
        if capacity is None:
            if stream is not None and stream != torch.cuda.current_stream():
                stream.synchronize()
            cap = int(offsets[-1].item())   # the ONE synchronisation of the call: the exact size
        else:
            cap = int(capacity)
        counts = torch.empty(cap, dtype=torch.int32, device=dev) if cap else torch.zeros(1, dtype=torch.int32, device=dev)   # (the consumers take no NULL)
        status = torch.empty(max(B, 1), dtype=torch.int32, device=dev)[:B]
        a.counts, a.status, a.capacity = counts.data_ptr(), status.data_ptr(), cap
        check(lib.la3d_rle_encode(C.byref(a)), "la3d_rle_encode")
    _record(stream, runs, offsets, ws, counts, status, *keep)
    return counts, offsets, status


def rle_encode_bits(bits: MaskBits, capacity=None, stream=None, return_status: bool = False):
    """``MaskBits`` -> ``RleRuns`` on the GPU (C-ABI ``la3d_rle_encode_offsets`` + ``la3d_rle_encode``): ``binary_mask_to_rle``
    (reference src/download_coconut.py:167-175) for a batch - the planes of any packer (``pack_mask_bits``, ``pack_logits_bits``,
    ``pack_label_bits(...).bits``, ``pack_poly_bits``, ``pack_crop_bits``) become COCO run lengths without leaving the device: the
    fastest source of the fit, a few hundred bytes per instance, what ``fit_annotations_sharded`` ships and the annotation JSON stores
    (``rle_objects``).  The runs cover the image (``bits.H`` x ``bits.frame_width``): pad columns are never mask.
    ``capacity=None`` reads ``offsets[-1]`` back once - the call's ONLY host synchronisation - and allocates ``counts`` exactly;
    ``capacity=int`` never synchronises (the chain can be captured into a graph): an instance whose run list does not fit gets status 1
    and is not written, so ask for ``return_status=True`` then - ``(RleRuns, status int32 (B,))``: 0 ok, 1 no room, 2 the planes
    changed between the two stages."""
    if not isinstance(bits, MaskBits):
        raise ValueError("rle_encode_bits: bits must be a MaskBits (pack_mask_bits, pack_logits_bits, pack_label_bits(...).bits, ...)")
    _rle_capacity("rle_encode_bits", capacity)
    mb = _mask_bits(bits)
    B, dev = int(mb.bits.shape[0]), mb.bits.device
    a = _lib.RleEncodeArgs(struct_size=C.sizeof(_lib.RleEncodeArgs), B=B, H=mb.H, W=mb.W, frame_width=0 if mb.frame_width == mb.W else mb.frame_width,
                           mask_bits=mb.bits.data_ptr(), bits_plane_stride=_bits_stride(mb.bits, B, mb.H, mb.W))
    counts, offsets, status = _rle_encode_run(a, B, dev, capacity, stream, [mb.bits])
    runs = RleRuns(counts, offsets, mb.H, mb.frame_width)
    return (runs, status) if return_status else runs


def rle_encode(masks, device=None, stream=None) -> RleRuns:
    """(B,H,W) bool / uint8 masks, on the host or the device -> ``RleRuns`` on the GPU: ``pack_mask_bits``, then ``rle_encode_bits``
    (one host synchronisation, for the exact size)."""
    return rle_encode_bits(pack_mask_bits(masks, frame_pad=True, device=device, stream=stream), stream=stream)


def rle_objects(runs, compress: bool = False, sizes=None) -> list:
    """Run lengths on the device -> the list of COCO RLE objects of the annotation JSON, ``{"size": [h, w], "counts": list}`` - or, with
    ``compress=True``, ``counts`` as the compressed ``str`` of ``rle_to_string``.  ``runs``: an ``RleRuns``; or the ``(counts, offsets)``
    of ``rle_encode_bits_frames`` with its ``sizes`` (B, 2).  ONE device-to-host copy (offsets, sizes and counts in one buffer)."""
    if isinstance(runs, tuple) and len(runs) == 4:
        counts, offsets, H, W = runs
    elif isinstance(runs, tuple) and len(runs) == 2 and sizes is not None:
        counts, offsets, H, W = runs[0], runs[1], None, None
    else:
        raise ValueError("rle_objects takes an RleRuns, or (counts, offsets) with sizes=")
    if isinstance(counts, torch.Tensor) and counts.is_cuda:
        B = int(offsets.numel()) - 1
        parts = [offsets.to(counts.device).to(torch.int64).reshape(-1), counts.to(torch.int64).reshape(-1)]
        if sizes is not None:
            parts.insert(1, torch.as_tensor(sizes).to(counts.device).to(torch.int64).reshape(-1))
        host = torch.cat(parts).cpu().numpy()
        offs = host[:B + 1]
        sz = host[B + 1:3 * B + 1].reshape(B, 2) if sizes is not None else None
        cnt = host[(3 * B + 1) if sizes is not None else (B + 1):]
    else:
        offs, cnt = np.asarray(offsets, np.int64).reshape(-1), np.asarray(counts, np.int64).reshape(-1)
        sz = None if sizes is None else np.asarray(sizes.cpu() if isinstance(sizes, torch.Tensor) else sizes, np.int64).reshape(-1, 2)
    out = []
    for n in range(len(offs) - 1):
        c = cnt[offs[n]:offs[n + 1]]
        out.append({"size": [int(H), int(W)] if sz is None else [int(sz[n, 0]), int(sz[n, 1])],
                    "counts": rle_to_string(c) if compress else c.tolist()})
    return out


def rle_encode_bits_frames(frames, bits: FrameBits, capacity=None, stream=None, return_status: bool = False):
    """``rle_encode_bits`` for the planes of images of DIFFERENT sizes (the frames form of C-ABI ``la3d_rle_encode_offsets`` +
    ``la3d_rle_encode``): ``frames`` - a ``PackedFrames`` / ``PackedFrames16`` / ``PackedLabels`` / ``PackedMasks`` whose frame table
    the planes were laid out for (another table: ValueError before any device work) -, ``bits`` the ``FrameBits`` of a frames packer.
    The runs of instance n are column-major over its OWN image, ``(H_p, W_p)`` unpadded.  Returns ``((counts, offsets), sizes)`` -
    ``(counts int32, offsets int64 (B+1,))`` on the GPU is what ``fit_instances_frames(rles=...)`` and ``pack_rle_bits_frames`` take;
    ``sizes`` int32 (B, 2) on the GPU holds the (h, w) of every instance (-1, -1 for a row whose image index lies outside the table;
    ``rle_objects((counts, offsets), sizes=sizes)`` writes the JSON objects) - and, with ``return_status=True``, ``status`` int32 (B,)
    as a third item: 0, 1 = no room in ``capacity``, 2 = the planes changed between the stages, 5 = a row whose image index, frame row
    or plane offset breaks the contract (it gets no runs - decided on the device, never an exception).  ``capacity`` as in
    ``rle_encode_bits``: None synchronises once for the exact size, an int never does.  ``frames`` may also be a ``FrameGrid``: with
    ``scaled_frames(frames, s)`` the planes ``open_bits_frames`` made at ``upscale=s`` are encoded."""
    who = "rle_encode_bits_frames"
    _rle_capacity(who, capacity)
    _tabled(who, frames, bits)
    dev = _on_gpu(frames.table, bits.bits)
    B, P = int(bits.offsets.numel()), int(frames.table.shape[0])
    if B and not P:
        raise ValueError(f"{who}: instances without a frame table")
    ii = _as_dev(bits.image_index, torch.int32, dev)
    a = _lib.RleEncodeArgs(struct_size=C.sizeof(_lib.RleEncodeArgs), B=B, H=max(int(frames.H), 1), W=max(int(frames.W), 1), P=P,
                           mask_bits=bits.bits.data_ptr(), frames=frames.table.data_ptr() if P else None, image_index=ii.data_ptr() if P else None,
                           bits_offsets=bits.offsets.data_ptr() if P else None)
    counts, offsets, status = _rle_encode_run(a, B, dev, capacity, stream, [frames.table, bits.bits, bits.offsets, ii])
    with torch.cuda.device(dev):
        if P:
            ok = (ii >= 0) & (ii < P)
            hw = frames.table[ii.clamp(0, P - 1).long()][:, [2, 4]]   # (the la3d_frame words: H, frame_width)
            sizes = torch.where(ok[:, None], hw, torch.full_like(hw, -1))
        else:
            sizes = torch.zeros((0, 2), dtype=torch.int32, device=dev)
    return ((counts, offsets), sizes, status) if return_status else ((counts, offsets), sizes)
