"""Annotation ingestion on the device: the data format immediately upstream of the box fit - COCO run lengths and
polygons, their decoders, filters and the fits that take them (host-side packing - ``pack_rle``, ``pack_polygons`` -: ``segm``).

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

The other sources live in modules of their own (``bits``, ``labels``, ``depth16``, ``frames``; plane operations in ``morph`` and
``rle_encode``) and this module is their facade: every name that was ever importable from here is imported below.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np
import torch

from . import _lib
from ._device import _as_dev, _dev, _plane_source, _ptr, _record, _stream, _upload_many  # noqa: F401
from ._lib import AUX, BOX_FILTERED, REC, check, lib
from .batched import Depth16, InstanceFitter, _bits_stride, _depth16_block, _depth16_check, _fit_args, height_rule_code, pad_depth_rows, padded_width, refuse_depth16  # noqa: F401
from .bits import (_LOGIT_DTYPES, MaskBits, _annotation_bits_plan, _bits_out, _crop_place, _crop_source, _crop_threshold, _mask_bits, _pack_annotation_bits,  # noqa: F401
                   _PackedBits, DepthGateStats, crop_placement, depth_gate_stats, fit_instances_bits, gate_depth_bits, mask_stats_bits, pack_crop_bits, pack_logits_bits, pack_mask_bits, pack_poly_bits, pack_rle_bits, unpack_mask_bits)
from .depth16 import _D16_DTYPES, pack_depth16, unpack_depth16  # noqa: F401
from .depth_align import masked_ratio_median  # noqa: F401
from .fitcall import depth_rows, depth_rows_for_bits, fit_call, mask_source  # noqa: F401
from .frames import (FRAME_DTYPE, MASKS_U8, FrameBits, PackedFrames, PackedFrames16, PackedLabels, PackedMasks, fit_instances_frames, fit_instances_frames_bits,  # noqa: F401
                     fit_instances_frames_labels, fit_instances_frames_masks, frame_bits_offsets, frame_table, pack_crop_bits_frames, pack_frames, pack_label_bits_frames,
                     pack_label_frames, pack_mask_bits_frames, pack_mask_frames, pack_poly_bits_frames, pack_rle_bits_frames, pack_rle_frames)
from .labels import _LABEL_NUMPY, _LABEL_TORCH, LabelBits, _label_planes, _label_rows, _label_source, fit_instances_labels, label_instances, pack_label_bits  # noqa: F401
from .morph import _gate_scalars, _open_args, _open_run, _open_scalars, bits_rects, crop_params, depth_gate_stats_frames, gate_depth_bits_frames, open_bits, select_crops  # noqa: F401
from .rle_encode import RleRuns, _rle_capacity, _rle_encode_run, rle_encode, rle_encode_bits, rle_encode_bits_frames, rle_objects, rle_to_string  # noqa: F401
from .segm import _rle_counts, pack_polygons, pack_rle, rle_from_string  # noqa: F401


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
