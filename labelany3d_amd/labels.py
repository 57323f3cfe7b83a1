"""Masks as label maps (include/la3d.h "masks as label maps"): one plane of segment ids per image -> the bit planes of its (image, id)
rows (``LabelBits``, ``pack_label_bits``), the fit that takes them (``fit_instances_labels``) and the ids a label map holds
(``label_instances``).  ``masks`` re-exports the public names."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from ._device import _as_dev, _dev, _ptr, _record, _stream, _upload_many
from .batched import _bits_stride, height_rule_code, padded_width
from .bits import MaskBits, _bits_out, fit_instances_bits


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
