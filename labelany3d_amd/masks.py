"""Mask ingestion on the device: the data format immediately upstream of the box fit.

The reference turns COCO / COCONut annotations into ``(N,H,W)`` bool arrays on the CPU with pycocotools
(``mask_utils.decode``, reference src/util.py:367,401-402; encoder src/download_coconut.py:167-175) and keeps
an instance when ``height/H > 0.0625 and not truncated and area >= 100`` (src/util.py:291-335, :375).  Here the
run lengths go to the GPU as they are (a few hundred bytes per instance instead of H*W bytes):

    counts, offsets, H, W = pack_rle(annotation_segmentations)        # host: list of COCO RLE dicts
    boxes, status, aux = fit_instances_rle(depth, (counts, offsets, H, W), K, ...)   # no dense mask at all
    masks = rle_decode((counts, offsets, H, W))                         # the reference's mask array, on the GPU
    keep  = keep_instances(mask_stats(masks), H, from_rle=True)         # the reference's three filters

Polygon segmentations — what every kept COCONut instance carries (the converter writes polygons for all non-crowd
instances, src/download_coconut.py:275-280) — take ``create_boolean_mask_from_polygon`` in the reference
(``cv2.fillPoly`` per part, src/util.py:386-400); here the parts go to the GPU as int32 vertex lists:

    polys = pack_polygons([a["segmentation"] for a in annos], H, W)    # host: truncation to int32 like :398
    boxes, status, aux = fit_instances_poly(depth, polys, K, ...)       # rasterised inside the fit kernel
    masks = poly_decode(polys)                                          # the reference's boolean masks, on the GPU
    keep  = keep_instances(mask_stats_poly(polys), H, from_rle=False)   # height = last row - first row + 1 (:328-335)

These, bit planes (``MaskBits``), label maps (``LabelBits``) and 16-bit depth (``pack_depth16``) are the sources of ONE frame size per
call; images of different sizes (``pack_frames``, ``fit_instances_frames*``) live in ``frames`` and are re-exported at the end.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import itertools
import threading
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import AUX, BOX_FILTERED, REC, check, lib
from .batched import (Depth16, InstanceFitter, _as_dev, _bits_stride, _depth16_block, _depth16_check, _dev, _fit_args, _ptr, _record,
                      _stream, _upload_many, height_rule_code, pad_depth_rows, padded_width, refuse_depth16)
from .fitcall import depth_rows, depth_rows_for_bits, fit_call, mask_source


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


def rle_decode(rles, device=None, stream=None) -> torch.Tensor:
    """``mask_utils.decode`` for a batch: (B,H,W) bool tensor on the GPU."""
    counts, offsets, H, W = pack_rle(rles)
    dev = _dev(device)
    c, o = _as_dev(counts, torch.int32, dev), _as_dev(offsets, torch.int64, dev)
    B = o.numel() - 1
    out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.la3d_rle_decode(_ptr(c), _ptr(o), B, H, W, _ptr(out), _stream(stream)), "la3d_rle_decode")
    return out.view(torch.bool)


def mask_stats(masks, boundary_threshold: int = 10, stream=None) -> torch.Tensor:
    """(B,4) int32 on the GPU: area, rows holding a pixel, last-first+1 rows, boundary-strip pixels — what the
    reference's analyze_mask / get_maximum_height / RLE-height look at (src/util.py:291-335, :368-369)."""
    dev = masks.device if isinstance(masks, torch.Tensor) and masks.is_cuda else _dev()
    m = _as_dev(masks, torch.uint8, dev)
    B, H, W = m.shape
    out = torch.empty((B, 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.la3d_mask_stats(_ptr(m), B, H, W, int(boundary_threshold), _ptr(out), _stream(stream)), "la3d_mask_stats")
    return out


def mask_stats_rle(rles, boundary_threshold: int = 10, stream=None, device=None) -> torch.Tensor:
    """``mask_stats`` straight from COCO run lengths (a list of RLE objects or the tuple from ``pack_rle``): the four
    filter quantities by interval arithmetic on the runs, no mask plane is decoded.  With ``keep_instances(...,
    from_rle=True)`` this is the reference's RLE branch of read_bounding_boxes_segmentations (src/util.py:364-376)."""
    counts, offsets, H, W = pack_rle(rles)
    dev = _dev(device)
    c, o = _as_dev(counts, torch.int32, dev), _as_dev(offsets, torch.int64, dev)
    B = o.numel() - 1
    out = torch.empty((B, 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.la3d_mask_stats_rle(_ptr(c), _ptr(o), B, H, W, int(boundary_threshold), _ptr(out), _stream(stream)),
              "la3d_mask_stats_rle")
    return out


def keep_instances(stats: torch.Tensor, image_height: int, from_rle: bool = True, scale_threshold: int = 100) -> torch.Tensor:
    """The reference's keep rule (src/util.py:375): height/H > 0.0625 and truncation < 10 and area >= 100, with
    height = rows holding a pixel for RLE annotations (:368-369) and last-first+1 for polygons (:328-335)."""
    height = stats[:, 1] if from_rle else stats[:, 2]
    return (height.double() / image_height > 0.0625) & (stats[:, 3] < 10) & (stats[:, 0] >= scale_threshold)


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


def _poly_dev(polys, dev):
    xy, ro, ir, H, W = polys
    return (_as_dev(xy, torch.int32, dev), _as_dev(ro, torch.int64, dev), _as_dev(ir, torch.int64, dev), H, W)


def poly_decode(polys, device=None, stream=None) -> torch.Tensor:
    """``create_boolean_mask_from_polygon`` (reference src/util.py:386-400) for a batch: (B,H,W) bool tensor on the GPU.
    ``polys`` is the tuple from ``pack_polygons``."""
    dev = _dev(device)
    xy, ro, ir, H, W = _poly_dev(polys, dev)
    B = ir.numel() - 1
    out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.la3d_poly_decode(_ptr(xy), _ptr(ro), _ptr(ir), B, H, W, _ptr(out), _stream(stream)), "la3d_poly_decode")
    return out.view(torch.bool)


def mask_stats_poly(polys, boundary_threshold: int = 10, stream=None, device=None) -> torch.Tensor:
    """``mask_stats`` for polygon annotations, rasterised in LDS (no plane is written).  With ``keep_instances(...,
    from_rle=False)`` this is the polygon branch of read_bounding_boxes_segmentations (src/util.py:371-376)."""
    dev = _dev(device)
    xy, ro, ir, H, W = _poly_dev(polys, dev)
    B = ir.numel() - 1
    out = torch.empty((B, 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.la3d_mask_stats_poly(_ptr(xy), _ptr(ro), _ptr(ir), B, H, W, int(boundary_threshold), _ptr(out), _stream(stream)),
              "la3d_mask_stats_poly")
    return out


def filter_annotations(annotations, image_size, boundary_threshold: int = 10, scale_threshold: int = 100, device=None):
    """The reference's ``read_bounding_boxes_segmentations(annotations, image_size)`` (src/util.py:336-383) without ever
    materialising a mask plane: crowd annotations are skipped (:355-357); RLE segmentations take ``mask_stats_rle`` with
    height = rows holding a pixel (:364-369), polygon segmentations take ``mask_stats_poly`` with height = last row - first
    row + 1 (``create_boolean_mask_from_polygon`` -> ``get_maximum_height``, :371-372, :328-335); the keep rule is :375
    (height/H > 0.0625, fewer than 10 boundary pixels, area >= 100).

    annotations: list of COCO annotation dicts with 'iscrowd', 'bbox', 'category_id' and a 'segmentation' that is an RLE
    ({'size': [h, w], 'counts': list | str | bytes}) or a list of polygon parts; image_size = (width, height) as in the
    reference.  Returns ``(bboxes, segmentations, kept_index, category_ids)``: the kept annotations' boxes, their
    segmentations in annotation order (RLE dicts -> ``fit_instances_rle`` / ``rle_decode``; part lists ->
    ``fit_instances_poly`` / ``poly_decode``; a mixed list -> ``segmentations_to_masks``), their positions in
    ``annotations`` and their raw COCO category ids (the reference maps those to super-category names with a table that is
    not part of this path)."""
    W_img, H_img = int(image_size[0]), int(image_size[1])
    keep = {}
    for kind, (idx, segs) in split_annotations(annotations).items():
        if not idx:
            continue
        st = (mask_stats_rle(segs, boundary_threshold, device=device) if kind == "rle"
              else mask_stats_poly(pack_polygons(segs, H_img, W_img), boundary_threshold, device=device))
        k = keep_instances(st, H_img, from_rle=kind == "rle", scale_threshold=scale_threshold).cpu().numpy()
        keep.update({i: (bool(f), c) for i, f, c in zip(idx, k, segs)})
    kept = [i for i in sorted(keep) if keep[i][0]]
    return ([annotations[i]["bbox"] for i in kept], [keep[i][1] for i in kept], np.asarray(kept, np.int64),
            [annotations[i]["category_id"] for i in kept])


def fit_instances_ex(depth, K, masks=None, rles=None, polys=None, ground=None, sample_idx=None, image_index=None, filter=None,
                     image_size=None, area_hint=None, stream=None, device=None, frame_width=None, _fitter=None, _stats=None,
                     method: str = "pca"):
    """Every option of the fit in one call (C-ABI ``la3d_fit_instances_ex``): exactly one of ``masks`` (B,H,W) u8 / bool,
    ``rles`` (COCO RLE list or ``pack_rle`` tuple), ``polys`` (``pack_polygons`` tuple) gives the masks; ``filter`` as in
    ``fit_instances_poly`` (run-length / polygon masks only); ``image_size=(width, height)`` adds the 2-D boxes the reference's
    Omni3D writer derives from every record - ``bbox2D_proj | bbox2D_trunc`` (B,8), src/tools/combine_results.py:105-108, :238-252 -
    written by the same kernel epilogue that writes the record.  ``area_hint`` (B,) int: mask areas the caller already knows (the
    annotation's ``area``, a preceding filter's statistics) - the size-balanced launch order then skips its estimate pass over the
    masks; a hint only orders the work.  ``frame_width`` (run-length / polygon masks): None - a frame whose width is not a multiple
    of 32 has its depth rows padded here (``pad_depth_rows``); an int - ``depth`` already IS padded (its last dimension is the padded
    width) and the masks' frame is ``frame_width`` columns wide.  ``method``: "pca" | "convex_hull" (see ``fit_instances``).
    Returns a dict: boxes, status, aux, and stats / boxes2d when asked."""
    _lib.method_code(method)   # (the reference's error for an unknown method, before any device work)
    is16 = isinstance(depth, Depth16)   # 16-bit planes, fitted where they lie (C-ABI ``la3d_fit_instances_depth16``)
    if is16:
        _depth16_check(depth)
        if frame_width is None and depth.frame_width:
            frame_width = int(depth.frame_width)
    dev = _dev(device)
    if (masks is not None) + (rles is not None) + (polys is not None) != 1:
        raise ValueError("give exactly one of masks / rles / polys")
    # (a host image_index is range-checked on the host as the caller gave it: ``given_index`` below; it goes up with the masks here)
    src, ground, ii, sample_idx, area_hint = mask_source(dev, masks=masks, rles=None if rles is None else pack_rle(rles), polys=polys,
                                                         small=(ground, image_index, sample_idx, area_hint))
    if filter and masks is not None:
        raise ValueError("the fused filter needs run-length or polygon masks")
    H, W, fw = src.H, src.W, 0
    if masks is None:
        if frame_width is None:   # rows of a width that is no multiple of 32 are padded here
            if is16 and W % 32 != 0:
                _depth16_check(depth, (H, W), f"the {src.what} frame")
            stored = padded_width(W)
        else:                     # the depth IS padded already: its last dimension is the stored width
            if int(frame_width) != W:
                raise ValueError(f"frame_width {frame_width} does not match the {src.what} frame width {W}")
            stored = int((depth.data if is16 else depth).shape[-1])
            if stored != W and (stored < W or stored % 32 != 0):
                raise ValueError("padded depth rows must be a multiple of 32 wide and at least frame_width")
        depth, fw = depth_rows(depth, stored, W, dev, pad=frame_width is None)
        W = stored
    # (_fitter / _stats: buffers a per-image caller keeps between calls - fit_annotations - instead of allocating them per call)
    return fit_call(src, depth, K, dev, H, W, image_index=ii, ground=ground, sample_idx=sample_idx, area_hint=area_hint, filter=filter,
                    image_size=image_size, stream=stream, method=method, frame_width=fw, given_index=image_index, fitter=_fitter,
                    stats=_stats)


_ANN_CACHE: dict = {}   # (B, H, W, device) -> (InstanceFitter, stats, pinned read-back buffer): the per-image pattern repeats a few shapes


_ANN_LOCK = threading.Lock()


def _ann_buffers(B, H, W, dev, kind, method="pca"):
    # per THREAD: two threads calling fit_annotations with equal shapes must not share a fitter, its statistics
    # buffer and its pinned read-back buffer; the dict itself is guarded by a lock
    key = (B, H, W, kind, dev.index if dev.index is not None else torch.cuda.current_device(), threading.get_ident(), method)
    with _ANN_LOCK:
        ent = _ANN_CACHE.get(key)
        if ent is None and len(_ANN_CACHE) >= 64:
            _ANN_CACHE.pop(next(iter(_ANN_CACHE)))
    if ent is None:
        f = InstanceFitter(B, H, W, dev, method=method)
        # the pinned buffer mirrors the head of the fitter's arena: boxes | aux | status (256-aligned pieces), without the workspace
        ent = (f, torch.empty((B, 4), dtype=torch.int32, device=dev), torch.empty(f._arena.numel() - f.workspace.numel(), dtype=torch.uint8, pin_memory=True))
        with _ANN_LOCK:
            _ANN_CACHE[key] = ent
    return ent


def fit_annotations(annotations, image_size, depth, K, ground=None, boundary_threshold: int = 10, scale_threshold: int = 100,
                    image_index=None, device=None, to_host: bool = False, method: str = "pca"):
    """``read_bounding_boxes_segmentations`` (reference src/util.py:336-383) and the box fit in ONE pass over the annotations:
    crowd annotations are skipped (:355-357); every other annotation's segmentation is decoded / rasterised once, inside the
    fit launch, which also evaluates the keep rule (:375) on the bit image and fits only the kept instances (``filter=`` of
    ``fit_instances_rle`` / ``fit_instances_poly``).  One launch per segmentation kind present.

    depth / K / image_index as in ``fit_instances`` (image_index per ANNOTATION when depth holds several planes); ground: None
    or (len(annotations), 4).  Returns ``(bboxes, kept_index, category_ids, boxes (n,39) f64, status (n,) i32)`` for the kept
    annotations in annotation order, the last two on the GPU - or, with ``to_host=True``, as NumPy arrays taken from the ONE
    packed read-back (records | aux | status in a single copy into pinned memory) that the keep decision needs anyway: no
    further device work, which is what a caller writing JSON wants.  Output buffers, workspace and the pinned buffer are kept per
    (B, H, W) between calls (the per-image pattern repeats a handful of shapes).  ``method``: "pca" | "convex_hull" (see
    ``fit_instances``)."""
    refuse_depth16(depth, "fit_annotations")
    _lib.method_code(method)   # (the reference's error for an unknown method, before any device work)
    W_img, H_img = int(image_size[0]), int(image_size[1])
    dev = _dev(device)
    split = split_annotations(annotations)
    flt = {"boundary_threshold": boundary_threshold, "scale_threshold": scale_threshold}
    if (to_host and isinstance(depth, torch.Tensor) and depth.is_cuda and depth.dtype == torch.float32 and depth.is_contiguous()
            and not isinstance(K, torch.Tensor) and not isinstance(ground, torch.Tensor) and not isinstance(image_index, torch.Tensor)):
        return _fit_annotations_host(annotations, split, W_img, H_img, depth, K, ground, image_index, flt, method)
    groups = _annotation_groups(annotations, ground, image_index, split=split)
    if padded_width(W_img) != W_img and groups:   # a frame of odd width: rows padded once for both segmentation kinds
        with torch.cuda.device(dev):
            depth, _ = pad_depth_rows(depth, dev)
    sels, box_all, st_all, pins = [], [], [], []
    for kind, sel, segs, g, ii, hint, _ in groups:
        # every small host array of the group goes up in ONE copy (six to eight separate uploads cost ~100 us per image)
        host = lambda v: None if isinstance(v, torch.Tensor) else v     # noqa: E731   (device tensors pass through as they are)
        packed = pack_rle(segs) if kind == "rle" else pack_polygons(segs, H_img, W_img)
        *arrays, Hh, Ww = packed
        *up, g_u, ii_u, hint_u, K_u = _upload_many(list(zip(arrays, (torch.int32, torch.int64, torch.int64))) + [
            (host(g), torch.float64), (host(ii), torch.int32), (hint, torch.int32), (host(K), torch.float64)], dev)
        fitter, stats_buf, pin = _ann_buffers(len(sel), Hh, padded_width(Ww), dev, kind, method)
        res = fit_instances_ex(depth, K_u if K_u is not None else K, ground=g_u if g_u is not None else g,
                               image_index=ii_u if ii_u is not None else ii, device=dev, filter=flt, area_hint=hint_u, _fitter=fitter,
                               _stats=stats_buf, frame_width=Ww, method=method, **{"rles" if kind == "rle" else "polys": (*up, Hh, Ww)})
        head = fitter._arena[:pin.numel()]
        pin.copy_(head, non_blocking=True)      # records | aux | status of this group: one copy, read after the one synchronisation
        sels.append(sel); box_all.append(res["boxes"]); st_all.append(res["status"]); pins.append((pin, len(sel)))
    if not sels:
        return [], np.zeros(0, np.int64), [], torch.zeros((0, 39), dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()          # the one synchronisation of the call
    up8 = lambda v: (v + 255) // 256 * 256  # noqa: E731  (InstanceFitter's arena layout)
    hb, hs = [], []
    for pin, n in pins:
        raw = pin.numpy()
        nb, na = n * REC * 8, n * AUX * 8
        hb.append(raw[:nb].view(np.float64).reshape(n, REC))
        hs.append(raw[up8(nb) + up8(na):up8(nb) + up8(na) + n * 4].view(np.int32))
    pos, st_host, head = _annotation_order(annotations, sels, hs)
    if to_host:
        bh = hb[0] if len(hb) == 1 else np.concatenate(hb)
        return head + (bh[pos].copy(), st_host[pos].copy())
    boxes_c = box_all[0] if len(box_all) == 1 else torch.cat(box_all)
    status_c = st_all[0] if len(st_all) == 1 else torch.cat(st_all)
    pt = torch.as_tensor(pos, device=dev)
    return head + (boxes_c.index_select(0, pt), status_c.index_select(0, pt))


def split_annotations(annotations):
    """Annotations by segmentation kind, as ``read_bounding_boxes_segmentations`` treats them (reference src/util.py:355-367):
    crowd annotations and annotations without a segmentation are skipped; a dict with ``counts`` is a run-length mask, anything
    else a list of polygon parts.  Returns {"rle": (indices, segmentations), "poly": (indices, segmentations)}."""
    groups = {"rle": ([], []), "poly": ([], [])}
    for i, a in enumerate(annotations):
        if a.get("iscrowd") or "segmentation" not in a:
            continue
        seg = a["segmentation"]
        kind = "rle" if isinstance(seg, dict) and "counts" in seg else "poly"
        groups[kind][0].append(i)
        groups[kind][1].append({"size": seg["size"], "counts": seg["counts"]} if kind == "rle" else seg)
    return groups


def area_hint_of(areas):
    """The ``area`` fields of a group of annotations (COCO: the mask area in pixels) as the ``area_hint`` of its fit call - it spares
    the launch order its estimate pass -, or None unless every annotation of the group has one."""
    return None if None in areas else np.clip(np.asarray(areas, dtype=np.float64), 0, 2**31 - 1).astype(np.int32)


def _annotation_groups(annotations, ground=None, image_index=None, dev=None, split=None):
    """THE walk over the annotations by segmentation kind (``split_annotations``): per kind present, ``(kind, sel, segmentations,
    ground rows, image_index rows, area_hint, sel_t)`` - ``sel`` the int64 annotation indices of the kind, the rows of ``ground`` /
    ``image_index`` they select (NumPy for host arrays; a tensor is indexed where it lies, or - ``dev`` given, as
    ``fit_annotations_all`` does - on ``dev``), the hint from the annotations' ``area``, and with ``dev`` the indices on it.  ``split``: the result of
    ``split_annotations`` where the caller has it already."""
    groups = []
    for kind, (idx, segs) in (split_annotations(annotations) if split is None else split).items():
        if idx:
            sel = np.asarray(idx, np.int64)
            sel_t = None if dev is None else torch.as_tensor(sel, device=dev)
            groups.append((kind, sel, segs, None if ground is None else _rows(ground, sel, sel_t),
                           None if image_index is None else _rows(image_index, sel, sel_t),
                           area_hint_of([annotations[i].get("area") for i in idx]), sel_t))
    return groups


def _rows(v, sel, sel_t):
    if not isinstance(v, torch.Tensor):
        return np.asarray(v)[sel]
    return v.to(sel_t.device)[sel_t] if sel_t is not None else v[torch.as_tensor(sel, device=v.device)]


def _annotation_order(annotations, sels, statuses):
    """The kept rows of per-kind results, back in annotation order: -> (positions in the concatenated results, the concatenated
    status, (bboxes, kept_index, category_ids)) - what ``fit_annotations`` returns ahead of the records."""
    sel_c = sels[0] if len(sels) == 1 else np.concatenate(sels)
    st = statuses[0] if len(statuses) == 1 else np.concatenate(statuses)
    pos = np.nonzero(st != BOX_FILTERED)[0]               # kept rows of the concatenated results ...
    pos = pos[np.argsort(sel_c[pos], kind="stable")]      # ... in annotation order
    kept = sel_c[pos]
    return pos, st, ([annotations[i]["bbox"] for i in kept], kept, [annotations[i]["category_id"] for i in kept])


def annotation_areas(annotations, default: float = 0.0) -> np.ndarray:
    """The ``area`` field of every annotation (COCO: the mask area in pixels) - the per-instance cost ``plan_shards`` balances by,
    known from the annotation file alone."""
    return np.asarray([float(a.get("area", default) or default) for a in annotations], dtype=np.float64)


def fit_annotations_all(annotations, image_size, depth, K, ground=None, image_index=None, filter=None, device=None,
                        method: str = "pca"):
    """The fit of ``fit_annotations`` with one record per ANNOTATION, in annotation order, on the GPU: ``(boxes (n,39) f64,
    status (n,) i32)``.  Skipped annotations (crowd, no segmentation) and - with ``filter`` (a dict of ``boundary_threshold`` /
    ``scale_threshold``, or True for the reference's 10 / 100) - the ones the keep rule drops carry status 6 and a NaN record.
    One launch per segmentation kind present; the segmentations are decoded / rasterised inside the fit kernel (no u8 plane
    exists anywhere).  This is the rank-local step of ``shard.fit_annotations_sharded``.  ``method``: "pca" | "convex_hull"."""
    refuse_depth16(depth, "fit_annotations_all")
    _lib.method_code(method)   # (the reference's error for an unknown method, before any device work)
    W_img, H_img = int(image_size[0]), int(image_size[1])
    dev = _dev(device)
    n = len(annotations)
    boxes = torch.full((n, REC), float("nan"), dtype=torch.float64, device=dev)
    status = torch.full((n,), int(BOX_FILTERED), dtype=torch.int32, device=dev)
    flt = None
    if filter:
        flt = {"boundary_threshold": 10, "scale_threshold": 100} if filter is True else dict(filter)
    groups = _annotation_groups(annotations, ground, image_index, dev)
    if W_img % 32 != 0 and groups:   # a frame of odd width: rows padded once for both kinds
        with torch.cuda.device(dev):
            depth, _ = pad_depth_rows(depth, dev)
    for kind, _, segs, g, ii, hint, sel_t in groups:
        kw = dict(rles=segs) if kind == "rle" else dict(polys=pack_polygons(segs, H_img, W_img))
        res = fit_instances_ex(depth, K, ground=g, image_index=ii, device=dev, filter=flt, area_hint=hint, frame_width=W_img,
                               method=method, **kw)
        boxes.index_copy_(0, sel_t, res["boxes"])
        status.index_copy_(0, sel_t, res["status"])
    return boxes, status


def _raw_stream(dev_index: int) -> int:
    """torch's current stream of a device as a hipStream_t value (the private accessor is ~10 x cheaper than building a Stream object:
    this sits on a ~100 us per-image path)."""
    try:
        return torch._C._cuda_getCurrentRawStream(dev_index)
    except AttributeError:
        return torch.cuda.current_stream(dev_index).cuda_stream


def _fit_annotations_host(annotations, split, W_img, H_img, depth, K, ground, image_index, flt, method="pca"):
    """``fit_annotations(to_host=True)`` with the depth plane(s) resident and everything else on the host: ONE foreign call per
    segmentation kind (``la3d_fit_annotations_host``: the small arrays go up through the library's pinned block, the records come back
    through it, the call polls a completion flag) - no torch tensor, no wrapper layers in between."""
    P = depth.shape[0] if depth.dim() == 3 else 1
    dev_index = depth.device.index if depth.device.index is not None else torch.cuda.current_device()
    Wp = padded_width(W_img)
    if Wp != W_img:   # a frame of odd width: rows padded to the next multiple of 32, frame_width says where the image ends
        depth, _ = pad_depth_rows(depth, depth.device)
    Kh = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(-1, 9))
    if Kh.shape[0] not in (1, P):
        raise ValueError("K must be (3,3) or (P,3,3)")
    groups = _annotation_groups(annotations, None, image_index, split=split)
    if not groups:
        return [], np.zeros(0, np.int64), [], np.zeros((0, REC)), np.zeros(0, np.int32)
    host = lambda v: None if v is None else v.ctypes.data   # noqa: E731
    # the C entry enqueues on the stream it is handed, on the thread's CURRENT device: the depth's device, and the stream the
    # depth (and the padding above) was produced on - torch's current stream of that device
    meth, stream, elsewhere = _lib.method_code(method), _raw_stream(dev_index), dev_index != torch.cuda.current_device()
    sels, recs, sts = [], [], []
    for kind, sel, segs, g, ii, hint, _ in groups:
        B = len(sel)
        if kind == "rle":
            counts, offsets, Hh, Ww = pack_rle(segs)
            masks_kw = dict(rle=(counts.ctypes.data, offsets.ctypes.data))
        else:
            xy, ro, ir, Hh, Ww = pack_polygons(segs, H_img, W_img)
            masks_kw = dict(poly=(xy.ctypes.data, ro.ctypes.data, ir.ctypes.data))
        if (Hh, Ww) != (H_img, W_img) or depth.shape[-2:] != (Hh, Wp):
            raise ValueError(f"depth {tuple(depth.shape[-2:])} / image size {(H_img, W_img)} do not match the mask size {(Hh, Ww)}")
        if ii is not None:
            ii = np.ascontiguousarray(ii, np.int32)
            if ii.size and (ii.min() < 0 or ii.max() >= P):
                raise ValueError("image_index out of range")
        elif P > 1:
            # one plane per ANNOTATION (crowd / unsegmented ones included): this kind's instances pick theirs by annotation index
            if P != len(annotations):
                raise ValueError("several depth planes need image_index (or one plane per annotation)")
            ii = sel.astype(np.int32)
        if ground is not None:
            g = np.ascontiguousarray(np.asarray(ground, dtype=np.float64).reshape(-1, 4)[sel])
        out = np.empty((B, REC), np.float64)
        st = np.empty(B, np.int32)
        a = _fit_args(B, Hh, Wp, depth.data_ptr(), P, Kh.ctypes.data, Kh.shape[0], out.ctypes.data, st.ctypes.data, None, None,
                      stream, image_index=host(ii), ground=host(g), area_hint=host(hint), filter=flt,
                      frame_width=Ww if Wp != Ww else 0, method=meth, **masks_kw)
        if elsewhere:
            with torch.cuda.device(dev_index):
                check(lib.la3d_fit_annotations_host(C.byref(a)), "la3d_fit_annotations_host")
        else:
            check(lib.la3d_fit_annotations_host(C.byref(a)), "la3d_fit_annotations_host")
        sels.append(sel); recs.append(out); sts.append(st)
    pos, st_c, head = _annotation_order(annotations, sels, sts)
    rec_c = recs[0] if len(recs) == 1 else np.concatenate(recs)
    return head + (rec_c[pos], st_c[pos])


def segmentations_to_masks(segmentations, H: int, W: int, device=None) -> torch.Tensor:
    """A list mixing RLE dicts and polygon part lists (what ``filter_annotations`` returns) -> (B,H,W) bool masks on the
    GPU in list order: the reference's ``np.array(segmentation_mask)`` (src/util.py:382)."""
    dev = _dev(device)
    out = torch.zeros((len(segmentations), H, W), dtype=torch.bool, device=dev)
    ri = [i for i, s in enumerate(segmentations) if isinstance(s, dict)]
    pi = [i for i, s in enumerate(segmentations) if not isinstance(s, dict)]
    if ri:
        out[torch.as_tensor(ri, device=dev)] = rle_decode([segmentations[i] for i in ri], device=dev)
    if pi:
        out[torch.as_tensor(pi, device=dev)] = poly_decode(pack_polygons([segmentations[i] for i in pi], H, W), device=dev)
    return out


def fit_instances_poly(depth, polys, K, ground=None, sample_idx=None, image_index=None, stream=None, device=None, filter=None,
                       method: str = "pca"):
    """fit_instances with polygon masks: the parts are rasterised inside the fit kernel, straight into its LDS bit image
    (cv2.fillPoly semantics, reference src/util.py:386-400).  Arguments and returns as ``labelany3d_amd.fit_instances``;
    ``polys`` is the tuple from ``pack_polygons``.

    PARITY UNPINNED until ``tests/golden/g16_fillpoly.npz`` exists: the rasteriser follows a restatement of OpenCV 4.x's fillPoly
    (oracle/poly_oracle.py), not outputs of cv2 itself - OpenCV cannot be installed in the build image.  Where it can:
    ``pip install opencv-python==4.10.0.84 && python tests/golden/make_golden_fillpoly.py``, then run the polygon tests.

    ``filter=True`` (or a dict of thresholds, see ``_filter_args``) fuses the reference's instance filter (src/util.py:375, polygon
    branch: height = last row - first row + 1) into the same launch: dropped instances get status 6 and a NaN record and cost no
    passes; a fourth return value holds the (B,4) statistics (area, rows, span, edge pixels) as ``mask_stats_poly`` gives them."""
    r = fit_instances_ex(depth, K, polys=polys, ground=ground, sample_idx=sample_idx, image_index=image_index, filter=filter,
                         stream=stream, device=device, method=method)
    return (r["boxes"], r["status"], r["aux"]) + ((r["stats"],) if filter else ())


def fit_instances_rle(depth, rles, K, ground=None, sample_idx=None, image_index=None, stream=None, device=None, filter=None,
                      method: str = "pca"):
    """fit_instances with run-length masks: the runs are decoded inside the fit kernel, straight into its LDS
    bit image.  Arguments and returns as ``labelany3d_amd.fit_instances``; ``rles`` is a list of COCO RLE
    objects or the tuple from ``pack_rle``.  ``filter``: as in ``fit_instances_poly`` (RLE branch of the rule: height = rows
    holding a pixel, src/util.py:368-369)."""
    r = fit_instances_ex(depth, K, rles=rles, ground=ground, sample_idx=sample_idx, image_index=image_index, filter=filter,
                         stream=stream, device=device, method=method)
    return (r["boxes"], r["status"], r["aux"]) + ((r["stats"],) if filter else ())


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


def _plane_source(x, dev, dtypes):
    """(B,H,W) input of a packer -> (tensor, plane stride in elements): a device tensor whose planes are dense (rows W apart, pixels
    adjacent) is read where it lies, whatever its plane stride and base alignment; everything else is made contiguous first."""
    if isinstance(x, torch.Tensor) and x.is_cuda and x.device == dev and x.dim() == 3 and x.dtype in dtypes:
        B, H, W = x.shape
        if (W == 1 or x.stride(2) == 1) and (H == 1 or x.stride(1) == W) and (B <= 1 or x.stride(0) >= H * W):
            t = x.view(torch.uint8) if x.dtype == torch.bool else x
            return t, (int(x.stride(0)) if B > 1 else H * W)
    t = _as_dev(x, dtypes[0] if not (isinstance(x, torch.Tensor) and x.dtype in dtypes) else x.dtype, dev)
    if t.dim() != 3:
        raise ValueError("expected (B,H,W)")
    return t, int(t.shape[1] * t.shape[2])


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


# ---- bit planes as run lengths (include/la3d.h "bit planes as run lengths") ----------------------------------------------------------
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


# ---- morphology on bit planes (include/la3d.h "morphology on bit planes") -------------------------------------------------------------
def _open_scalars(who: str, k, upscale) -> None:   # the k and upscale of an opening, of either form
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 31 or int(k) % 2 == 0:
        raise ValueError(f"{who}: k must be an odd int in 1 .. 31, not {k!r}")
    if isinstance(upscale, bool) or not isinstance(upscale, (int, np.integer)) or int(upscale) not in (1, 2, 4):
        raise ValueError(f"{who}: upscale must be 1, 2 or 4 (factors whose nearest-neighbour rule is u // s under every convention), not {upscale!r}")


def _gate_scalars(who: str, min_area, crop_size) -> None:   # the gate of select_crops, of either form
    if isinstance(min_area, bool) or not isinstance(min_area, (int, np.integer)) or int(min_area) < 0:
        raise ValueError(f"{who}: min_area must be an int >= 0, not {min_area!r}")
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


class LabelBits(NamedTuple):
    """What ``pack_label_bits`` makes of label maps: ``bits`` - the ``MaskBits`` of the B (image, id) rows -, ``image_index`` int32 (B,)
    on the GPU - the image of every row, what ``fit_instances_bits`` takes as ``image_index`` -, ``area`` int32 (B,) on the GPU - the
    pixel count of every plane (``area_hint``; ``draw_sample_idx(area)`` gives the reference's draws for subsample mode)."""
    bits: MaskBits
    image_index: torch.Tensor
    area: torch.Tensor


_LABEL_TORCH = {torch.uint8: _lib.LABEL_U8, torch.uint16: _lib.LABEL_U16, torch.int16: _lib.LABEL_U16, torch.int32: _lib.LABEL_I32}
_LABEL_NUMPY = {np.dtype(np.uint8): _lib.LABEL_U8, np.dtype(np.uint16): _lib.LABEL_U16, np.dtype(np.int16): _lib.LABEL_U16,
                np.dtype(np.int32): _lib.LABEL_I32}


def _label_planes(labels, rgb: bool):
    """The argument checks of a label map that need no device: -> (labels as (P,H,W[,3]), element code, P, H, W)."""
    if isinstance(labels, torch.Tensor):
        code = _LABEL_TORCH.get(labels.dtype)
    else:
        labels = np.asarray(labels)
        code = _LABEL_NUMPY.get(labels.dtype)
    if code is None:
        raise ValueError(f"label maps must be uint8, uint16, int16 (read as uint16) or int32, not {labels.dtype}")
    nd = labels.ndim
    if rgb:
        if code != _lib.LABEL_U8:
            raise ValueError(f"rgb=True takes uint8 label maps, not {labels.dtype}")
        if nd not in (3, 4) or labels.shape[-1] != 3:
            raise ValueError(f"rgb=True takes (P,H,W,3) or (H,W,3) label maps, not {tuple(labels.shape)}")
        code = _lib.LABEL_RGB8
        if nd == 3:
            labels = labels[None]
    else:
        if nd not in (2, 3):
            raise ValueError(f"label maps must be (P,H,W) or (H,W), not {tuple(labels.shape)}")
        if nd == 2:
            labels = labels[None]
    P, H, W = (int(n) for n in labels.shape[:3])
    if H <= 0 or W <= 0:
        raise ValueError(f"label maps of an empty frame {(H, W)}")
    return labels, code, P, H, W


def _label_rows(ids, P: int):
    """``ids`` of ``pack_label_bits`` -> (inst_label, inst_offsets, image_index, B): host int32 arrays where ``ids`` came on the host
    (checked here), device tensors as they are (image_index is then left to the device: None)."""
    if isinstance(ids, tuple) and len(ids) == 2:   # (a TUPLE of two is the flat form; per-image ids of two images come as a list)
        lab, off = ids
        if isinstance(lab, torch.Tensor) and lab.is_cuda or isinstance(off, torch.Tensor) and off.is_cuda:
            if not (isinstance(lab, torch.Tensor) and isinstance(off, torch.Tensor) and lab.is_cuda and off.is_cuda):
                raise ValueError("(inst_label, inst_offsets) must both be host arrays or both be device tensors")
            if lab.dim() != 1 or off.dim() != 1 or off.numel() != P + 1:
                raise ValueError(f"inst_label must be (B,) and inst_offsets (P+1,) = ({P + 1},)")
            return lab, off, None, int(lab.numel())
        lab = np.asarray(lab.numpy() if isinstance(lab, torch.Tensor) else lab).astype(np.int64).reshape(-1)
        off = np.asarray(off.numpy() if isinstance(off, torch.Tensor) else off).astype(np.int64).reshape(-1)
        if len(off) != P + 1:
            raise ValueError(f"inst_offsets must have P + 1 = {P + 1} entries, not {len(off)}")
    else:
        try:
            per = [np.asarray(x, dtype=np.int64).reshape(-1) for x in ids]
        except TypeError as e:
            raise ValueError("ids must be a sequence of P id sequences or a tuple (inst_label, inst_offsets)") from e
        if len(per) != P:
            raise ValueError(f"ids must hold one id sequence per image: {len(per)} given for {P} label maps")
        off = np.zeros(P + 1, np.int64)
        np.cumsum([len(x) for x in per], out=off[1:])
        lab = np.concatenate(per) if per else np.zeros(0, np.int64)
    B = len(lab)
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != B:
        raise ValueError(f"inst_offsets must start at 0, never decrease and end at B = {B}")
    if B and (lab.min() < -2**31 or lab.max() > 2**31 - 1):
        raise ValueError("ids must fit int32")
    return lab.astype(np.int32), off.astype(np.int32), np.repeat(np.arange(P, dtype=np.int32), np.diff(off)), B


def _label_source(labels, code, dev):
    """(P,H,W[,3]) label maps -> (device tensor, plane stride in elements / pixels): a resident tensor with dense planes is read where it
    lies (``_plane_source``'s rule), anything else is made contiguous and uploaded."""
    P, H, W = labels.shape[:3]
    c = 3 if code == _lib.LABEL_RGB8 else 1
    if isinstance(labels, torch.Tensor):
        t = labels.view(torch.int16) if labels.dtype == torch.uint16 else labels   # (bit patterns: uint16 has few kernels)
        if t.is_cuda and t.device == dev:
            st = t.stride()
            dense = (c == 1 or st[3] == 1) and (W == 1 or st[2] == c) and (H == 1 or st[1] == W * c)
            if dense and (P <= 1 or (st[0] >= H * W * c and st[0] % c == 0)):
                return t, (int(st[0]) // c if P > 1 else H * W)
        return t.to(dev).contiguous(), H * W
    a = np.ascontiguousarray(labels)
    return torch.as_tensor(a.view(np.int16) if a.dtype == np.uint16 else a, device=dev), H * W


def pack_label_bits(labels, ids, frame_pad: bool = True, rgb: bool = False, device=None, stream=None, out=None) -> LabelBits:
    """Label maps -> the bit planes of their instances (C-ABI ``la3d_pack_label_bits``): plane b is ``labels[image of b] == id of b``,
    in the format of ``pack_mask_bits``; the labels of an image are read once, however many instances it has.

    ``labels``: (P,H,W) or (H,W) ``torch.uint8`` / ``uint16`` / ``int16`` (read as uint16) / ``int32`` or a NumPy array of those; with
    ``rgb=True`` (P,H,W,3) / (H,W,3) uint8 - a COCO panoptic PNG as it decodes, id = R + 256 G + 65536 B.  A resident tensor with dense
    planes is read where it lies (any plane stride, any base alignment); anything else is made contiguous and uploaded.
    ``ids``: a sequence of P id sequences, one per image, possibly empty (``[[s["id"] for s in a["segments_info"]] for a in annos]``),
    or the tuple ``(inst_label (B,), inst_offsets (P+1,))`` of host arrays or device tensors - the instances of image p are the rows
    ``inst_offsets[p] .. inst_offsets[p+1]-1``.  Host ids go up in one copy and are checked; device tensors are taken as they are (the
    kernel touches no row outside [0, B) whatever they hold).  An id that is absent - or outside the dtype's range - gives an all-zero
    plane of area 0; a repeated id gives the plane again; an image without ids is never read.
    ``frame_pad`` / ``out`` as in ``pack_mask_bits``.  Returns ``LabelBits(bits, image_index, area)``.  No host synchronisation."""
    labels, code, P, H, W = _label_planes(labels, rgb)
    lab, off, ii, B = _label_rows(ids, P)
    if device is None and isinstance(labels, torch.Tensor) and labels.is_cuda:
        device = labels.device
    dev = _dev(device)
    W_out = padded_width(W) if frame_pad else W
    with torch.cuda.device(dev):
        x, ps = _label_source(labels, code, dev)
        if ii is not None:
            lab, off, ii = _upload_many([(lab, torch.int32), (off, torch.int32), (ii, torch.int32)], dev)
        else:
            lab, off = _as_dev(lab, torch.int32, dev), _as_dev(off, torch.int32, dev)
            # the image of every row from the offsets, on the device: the number of images whose rows end at or before b
            ii = torch.searchsorted(off[1:].contiguous(), torch.arange(B, dtype=torch.int32, device=dev), right=True).to(torch.int32)
        o = _bits_out(out, B, H, W_out, dev)
        area = torch.empty(B, dtype=torch.int32, device=dev)
        check(lib.la3d_pack_label_bits(_ptr(x), code, ps, P, H, W, W_out, _ptr(off), _ptr(lab), B, _ptr(o), _bits_stride(o, B, H, W_out),
                                       _ptr(area), _stream(stream)), "la3d_pack_label_bits")
    _record(stream, x, lab, off, ii, o, area)
    return LabelBits(MaskBits(o, H, W_out, W), ii, area)


def fit_instances_labels(depth, labels, ids, K, ground=None, sample_idx=None, filter=None, image_size=None, method: str = "pca",
                         height_rule: str = "rows", rgb: bool = False, stream=None, device=None):
    """The depth + mask fit of every listed instance of P label maps in one call: ``pack_label_bits`` (one pass over the labels), then
    ``fit_instances_bits`` with the rows' ``image_index`` and their exact areas as ``area_hint``.  ``depth``: (P,H,W) float32 - one plane
    per image - or a ``Depth16``; ``K``: (3,3) or (P,3,3); ``labels`` / ``ids`` / ``rgb`` as in ``pack_label_bits``; ``ground`` (B,4),
    ``sample_idx`` (B,500), ``filter``, ``image_size``, ``method`` ("pca" | "convex_hull", with the per-instance refusals of a hull
    call) and ``height_rule`` as in ``fit_instances_bits``, per (image, id) row in ``ids`` order.  Returns what ``fit_instances_bits``
    returns - boxes, status, aux[, stats][, boxes2d] - followed by the ``LabelBits``.  No host synchronisation: for subsample mode
    take the areas from ``label_instances`` (or ``segments_info``) and draw ``draw_sample_idx(areas)`` beforehand."""
    _lib.method_code(method)   # (the reference's error for an unknown method, before any device work)
    height_rule_code(height_rule)
    lb = pack_label_bits(labels, ids, frame_pad=True, rgb=rgb, device=device, stream=stream)
    res = fit_instances_bits(depth, lb.bits, K, ground=ground, sample_idx=sample_idx, image_index=lb.image_index, stream=stream,
                             device=lb.bits.bits.device, filter=filter, image_size=image_size, area_hint=lb.area, method=method,
                             height_rule=height_rule)
    return tuple(res) + (lb,)


def label_instances(labels, ignore=(0,), min_area: int = 1, rgb: bool = False):
    """The instances a label map holds, for callers without a ``segments_info`` (the output of a panoptic / entity segmentation
    network): ``(ids, areas)`` - per image a NumPy int32 array of the ids present, ascending, without those in ``ignore`` (0: the
    unlabeled id of COCO panoptic maps) and those of fewer than ``min_area`` pixels, and an int64 array of their pixel counts.
    ``labels`` / ``rgb`` as in ``pack_label_bits``, on the host or the device - or a sequence of maps of DIFFERENT sizes (what
    ``pack_label_frames`` takes), handled image by image.  Plumbing, not a hot path: one ``torch.unique`` over
    ``image << 32 | label`` keys where the labels lie, and it SYNCHRONISES (the result is read back).  ``draw_sample_idx(np.concatenate(
    areas))`` gives the reference's draws for subsample mode (``sample_idx`` of ``fit_instances_labels``)."""
    if isinstance(labels, (list, tuple)) and len({tuple(m.shape) for m in labels if hasattr(m, "shape")}) > 1:
        # maps of different sizes (what pack_label_frames takes): image by image
        ids, areas = [], []
        for m in labels:
            i, a = label_instances(m, ignore=ignore, min_area=min_area, rgb=rgb)
            ids += i
            areas += a
        return ids, areas
    labels, code, P, H, W = _label_planes(labels, rgb)
    t = labels if isinstance(labels, torch.Tensor) else torch.as_tensor(labels.view(np.int16) if labels.dtype == np.uint16 else labels)
    if t.dtype == torch.uint16:
        t = t.view(torch.int16)
    mask = {torch.uint8: 0xff, torch.int16: 0xffff, torch.int32: 0xffffffff}[t.dtype]
    t = t.to(torch.int64) & mask   # (zero-extended; an int32 label keeps its low 32 bits and gets its sign back below)
    if rgb:
        t = t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16)
    keys = (torch.arange(P, dtype=torch.int64, device=t.device)[:, None, None] << 32) | t
    u, c = torch.unique(keys, return_counts=True)
    u, c = u.cpu().numpy(), c.cpu().numpy()
    img, lab = u >> 32, (u & 0xffffffff).astype(np.uint32).view(np.int32)
    keep = (c >= int(min_area)) & ~np.isin(lab, np.asarray(list(ignore), dtype=np.int64).astype(np.int32) if len(ignore) else np.zeros(0, np.int32))
    ids, areas = [], []
    for p in range(P):
        sel = np.nonzero((img == p) & keep)[0]
        sel = sel[np.argsort(lab[sel], kind="stable")]
        ids.append(lab[sel].astype(np.int32))
        areas.append(c[sel].astype(np.int64))
    return ids, areas


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


def masked_ratio_median(depth_map, depth_render, mask, render_mask=None, image_index=None, stream=None):
    """Per instance ``np.median(depth_map[overlap] / depth_render[overlap])`` with ``overlap = mask & render_mask``
    — the scale estimate of the reference's align_to_depth_match (src/util.py:476-486), exact (radix select on
    the float32 ratios).  depth_map (P,H,W) or (H,W); depth_render, mask, render_mask (B,H,W).
    Returns (median float32 (B,), count int32 (B,)) on the GPU; an empty overlap gives count 0 and NaN (the
    reference returns the identity transform there, :476-478)."""
    dev = mask.device if isinstance(mask, torch.Tensor) and mask.is_cuda else _dev()
    m = _as_dev(mask, torch.uint8, dev)
    B, H, W = m.shape
    rm = None if render_mask is None else _as_dev(render_mask, torch.uint8, dev)
    d = _as_dev(depth_map, torch.float32, dev)
    if d.dim() == 2:
        d = d[None]
    r = _as_dev(depth_render, torch.float32, dev)
    ii = None if image_index is None else _as_dev(image_index, torch.int32, dev)
    if ii is None and d.shape[0] not in (1, B):
        raise ValueError("without image_index, depth_map must have 1 or B planes")
    med = torch.empty(B, dtype=torch.float32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.la3d_masked_ratio_median(_ptr(d), H * W if d.shape[0] > 1 else 0, _ptr(ii), _ptr(r), _ptr(m), _ptr(rm), B, H, W,
                                           _ptr(med), _ptr(cnt), _stream(stream)), "la3d_masked_ratio_median")
    return med, cnt


# the mixed-size ("frames") layer: its public names stay importable from here (last on purpose: frames imports from this module)
from .frames import (FRAME_DTYPE, MASKS_U8, FrameBits, PackedFrames, PackedFrames16, PackedLabels, PackedMasks, fit_instances_frames,  # noqa: E402,F401
                     fit_instances_frames_bits, fit_instances_frames_labels, fit_instances_frames_masks, frame_bits_offsets, frame_table,
                     pack_crop_bits_frames, pack_frames, pack_label_bits_frames, pack_label_frames, pack_mask_bits_frames, pack_mask_frames, pack_poly_bits_frames,
                     pack_rle_bits_frames, pack_rle_frames, rle_encode_bits_frames)
