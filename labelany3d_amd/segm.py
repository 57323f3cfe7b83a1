"""Host-side packing of COCO segmentations: run lengths and polygon parts as the flat NumPy arrays the device entries take."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np

from ._lib import lib


def rle_from_string(s) -> np.ndarray:
    """COCO compressed RLE string -> run lengths (pycocotools rleFrString), via the library's host helper."""
    if isinstance(s, str):
        s = s.encode("ascii")
    cap = len(s) + 1
    buf = (C.c_int32 * cap)()
    n = lib.la3d_rle_from_string_host(s, len(s), buf, cap)
    if n < 0:
        raise ValueError("malformed COCO RLE string")
    return np.frombuffer(buf, dtype=np.int32, count=n).copy()


def pack_rle(rles):
    """List of COCO RLE objects ({'size': [h, w], 'counts': list | str | bytes}, as in the annotation JSON the
    reference reads at src/util.py:360-368) -> (counts int32 (T,), offsets int64 (B+1,), H, W) NumPy arrays."""
    if isinstance(rles, tuple) and len(rles) == 4:
        return rles
    sizes = {tuple(r["size"]) for r in rles}
    if len(sizes) > 1:
        raise ValueError("all masks of one batch must share the frame size")
    H, W = sizes.pop() if sizes else (0, 0)
    counts, offsets = _rle_counts([r["counts"] for r in rles])
    return counts, offsets, int(H), int(W)


def _rle_counts(cs):
    """The ``counts`` of a batch of COCO RLE objects (lists, compressed strings, arrays) -> (counts int32 (T,), offsets int64 (B+1,));
    an empty batch gives one zero count (the kernels take no NULL)."""
    if cs and all(type(c) is list for c in cs):   # uncompressed run lengths as the JSON holds them: one conversion loop for the batch
        lens = np.fromiter(map(len, cs), np.int64, len(cs))
        counts = np.fromiter(itertools.chain.from_iterable(cs), np.int64, int(lens.sum())).astype(np.int32)
        offsets = np.zeros(len(cs) + 1, np.int64)
        np.cumsum(lens, out=offsets[1:])
    else:
        parts = [rle_from_string(c) if isinstance(c, (str, bytes)) else np.asarray(c, dtype=np.int32) for c in cs]
        offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        counts = np.concatenate(parts).astype(np.int32) if parts and offsets[-1] else np.zeros(1, np.int32)
    if not len(counts):
        counts = np.zeros(1, np.int32)
    return counts, offsets


def pack_polygons(segmentations, H=None, W=None):
    """List of polygon segmentations (each a list of parts, each part a flat [x0, y0, x1, y1, ...] list as in the COCO /
    COCONut JSON) -> ``(xy int32 (T,2), ring_offsets int64 (R+1,), inst_rings int64 (B+1,), H, W)``.  Vertices are
    truncated exactly like the reference: ``np.array(polygon).reshape(-1, 2).astype(np.int32)`` (src/util.py:398) — an odd
    number of coordinates raises the same ``ValueError`` from ``reshape``."""
    if isinstance(segmentations, tuple) and len(segmentations) == 5:
        return segmentations
    if H is None or W is None:
        raise ValueError("pack_polygons needs the frame size (H, W)")
    for seg in segmentations:
        if not isinstance(seg, (list, tuple)):
            raise TypeError("polygon segmentation must be a list of parts")
    parts = [polygon for seg in segmentations for polygon in seg]
    inst_rings = np.zeros(len(segmentations) + 1, np.int64)
    np.cumsum([len(seg) for seg in segmentations], out=inst_rings[1:])
    # (a part given as nested pairs [[x, y], ...] is a list too: the flat fast path is for lists of scalars only)
    plain = all(type(q) is list and not (q and isinstance(q[0], (list, tuple, np.ndarray))) for q in parts)
    lens = np.fromiter(map(len, parts), np.int64, len(parts)) if plain else None
    if plain and len(parts) and not (lens & 1).any():
        # flat Python lists (what the annotation JSON holds): ONE conversion loop over all coordinates of the batch instead of one
        # np.array per part (a third of the packing time of a 256-image batch); the truncation is the same astype
        flat = np.fromiter(itertools.chain.from_iterable(parts), np.float64, int(lens.sum()))
        xy = flat.reshape(-1, 2).astype(np.int32)
        ring_off = np.zeros(len(parts) + 1, np.int64)
        np.cumsum(lens >> 1, out=ring_off[1:])
    else:   # arrays, nested pairs, or an odd count (np.reshape raises the reference's ValueError)
        pts, ring = [], [0]
        for polygon in parts:
            q = np.array(polygon).reshape(-1, 2).astype(np.int32)
            pts.append(q)
            ring.append(ring[-1] + len(q))
        xy = np.concatenate(pts).astype(np.int32) if pts else np.zeros((0, 2), np.int32)
        ring_off = np.asarray(ring, np.int64)
    if not len(xy):
        xy = np.zeros((1, 2), np.int32)
    return xy, ring_off, inst_rings, int(H), int(W)
