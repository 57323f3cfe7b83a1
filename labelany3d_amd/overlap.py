"""Pairwise mask overlap on bit planes (include/la3d.h "mask overlap on bit planes"): the mask-level IoU matrix of every image and
the greedy mask NMS that reads it - what relates two planes of ONE image, for the planes of any packer (``MaskBits`` of one frame
size, ``FrameBits`` of images of different sizes).  The mask analogue of the box-level ``iou2d_matrix`` / ``hungarian_matching``."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from ._device import _record, _stream, _upload_many
from .batched import _bits_stride
from .frames import FrameBits, _on_gpu, _same_table
from .bits import MaskBits

TILE_DTYPE = np.dtype([(n, "<i8" if n == "out0" else "<i4") for n, _ in _lib.OverlapTile._fields_])
"""One row of the tile table of ``la3d_mask_overlap_plan``: ``la3d_overlap_tile`` of include/la3d.h (64 bytes)."""

_KINDS = {None: _lib.OVERLAP_NONE, "iou": _lib.OVERLAP_IOU, "iom": _lib.OVERLAP_IOM, "ioa": _lib.OVERLAP_IOA}


class MaskOverlap(NamedTuple):
    """What ``mask_overlap`` returns.  ``inter`` int32, flat, on the device: group g's matrix at ``[offsets[g], offsets[g + 1])``,
    row-major (row i of A, row j of B) - ``matrix(g)`` views it; ``iou`` float64 in the same layout, or None; ``area_a`` / ``area_b``
    int32 on the device, one per row of A / of B (the self form: the same tensor); ``offsets`` host int64 (G + 1,); ``counts_a`` /
    ``counts_b`` host int32 (G,).  A ``FrameBits`` row the device refuses has area -1, and every pair of it inter -1 and iou NaN."""
    inter: torch.Tensor
    iou: Optional[torch.Tensor]
    area_a: torch.Tensor
    area_b: torch.Tensor
    offsets: np.ndarray
    counts_a: np.ndarray
    counts_b: np.ndarray

    def matrix(self, g: int, what: str = "inter") -> torch.Tensor:
        """The ``(na_g, nb_g)`` view of group ``g``: ``what`` = "inter" or "iou"."""
        if what not in ("inter", "iou"):
            raise ValueError(f"matrix: what must be 'inter' or 'iou', not {what!r}")
        t = self.inter if what == "inter" else self.iou
        if t is None:
            raise ValueError("matrix: this overlap was computed without iou")
        g = int(g)
        if not 0 <= g < len(self.counts_a):
            raise ValueError(f"matrix: group {g} outside [0, {len(self.counts_a)})")
        return t[int(self.offsets[g]):int(self.offsets[g + 1])].view(int(self.counts_a[g]), int(self.counts_b[g]))


class OverlapPlan(NamedTuple):
    """The tables of one ``mask_overlap`` call shape (``mask_overlap_plan``): the host tile table, its device copy, the workspace, the
    output offsets, and what they were planned for.  Prepared once, it makes the call a pure enqueue (capturable)."""
    tiles_host: np.ndarray
    tiles: Optional[torch.Tensor]
    workspace: Optional[torch.Tensor]
    offsets: np.ndarray
    counts_a: np.ndarray
    counts_b: np.ndarray
    self_form: bool
    group_words: np.ndarray


def _counts(who: str, name: str, counts, rows: int) -> np.ndarray:
    try:
        c = np.asarray(list(counts) if not isinstance(counts, np.ndarray) else counts)
    except TypeError:
        raise ValueError(f"{who}: {name} must be a host sequence of ints") from None
    if isinstance(counts, torch.Tensor) or c.ndim != 1 or (c.size and not np.issubdtype(c.dtype, np.integer)):
        raise ValueError(f"{who}: {name} must be a host sequence of ints")
    if c.size and int(c.min()) < 0:
        raise ValueError(f"{who}: {name} must not hold a negative count")
    if int(c.sum()) != rows:
        raise ValueError(f"{who}: {name} sums to {int(c.sum())}, the planes have {rows} rows")
    return c.astype(np.int32)


def plan_tiles(counts_a, counts_b=None, group_words=None, nwords: int = 0):
    """C-ABI ``la3d_mask_overlap_plan`` on the host (no device): rows per group of A and of B (``counts_b`` None: the self form) and
    words per group (``group_words`` None: ``nwords`` for all) -> ``(tiles, offsets)``: the tile table as a ``TILE_DTYPE`` array and
    the int64 (G + 1,) output offsets.  Beyond the limits of the header: ``La3dError``."""
    ca = np.ascontiguousarray(counts_a, np.int32)
    cb = None if counts_b is None else np.ascontiguousarray(counts_b, np.int32)
    gw = None if group_words is None else np.ascontiguousarray(group_words, np.int64)
    G = len(ca)
    offsets = np.zeros(G + 1, np.int64)
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)   # noqa: E731
    n = int(lib.la3d_mask_overlap_plan(G, p(ca), p(cb), p(gw), int(nwords), None, 0, p(offsets)))
    if n < 0:
        check(n, "la3d_mask_overlap_plan")
    tiles = np.zeros(n, TILE_DTYPE)
    got = int(lib.la3d_mask_overlap_plan(G, p(ca), p(cb), p(gw), int(nwords), p(tiles) if n else None, n, p(offsets)))
    if got != n:
        check(got if got < 0 else -1, "la3d_mask_overlap_plan")
    return tiles, offsets


def _geometry(who: str, a, b, counts_a, counts_b, frames):
    """Every argument error of an overlap call, before any device work -> (frames form?, counts_a, counts_b | None, group_words |
    None, nwords)."""
    framed = isinstance(a, FrameBits)
    if not framed and not isinstance(a, MaskBits):
        raise ValueError(f"{who}: the planes must be a MaskBits or a FrameBits")
    if b is not None and type(b) is not type(a):
        raise ValueError(f"{who}: a and b must both be MaskBits or both be FrameBits")
    if b is None and counts_b is not None:
        raise ValueError(f"{who}: counts_b without b (the self form takes counts_a)")
    if framed:
        if frames is None or not all(hasattr(frames, f) for f in ("table", "table_host", "H", "W")):
            raise ValueError(f"{who}: FrameBits need frames, the packed object whose frame table the planes were laid out for")
        _same_table(frames, a)
        if b is not None:
            _same_table(frames, b)
        P = len(frames.table_host)
        if counts_a is None or (b is not None and counts_b is None):
            raise ValueError(f"{who}: FrameBits need counts, one entry per image of the table ({P})")
        rows_a, rows_b = int(a.offsets.numel()), None if b is None else int(b.offsets.numel())
    else:
        if frames is not None:
            raise ValueError(f"{who}: frames goes with FrameBits, not with MaskBits")
        for m in (a, b):
            if m is not None and not (isinstance(m.bits, torch.Tensor) and m.bits.dim() == 2 and 0 < int(m.frame_width) <= int(m.W) and int(m.H) > 0):
                raise ValueError(f"{who}: MaskBits must hold a (B, words) tensor and state a frame with 0 < frame_width <= W, H > 0")
        if b is not None and (int(a.H), int(a.W), int(a.frame_width)) != (int(b.H), int(b.W), int(b.frame_width)):
            raise ValueError(f"{who}: a and b state different frames: H, W, frame_width {(a.H, a.W, a.frame_width)} and {(b.H, b.W, b.frame_width)}")
        rows_a, rows_b = int(a.bits.shape[0]), None if b is None else int(b.bits.shape[0])
    ca = _counts(who, "counts_a", [rows_a] if counts_a is None else counts_a, rows_a)
    cb = None if b is None else _counts(who, "counts_b", [rows_b] if counts_b is None else counts_b, rows_b)
    if cb is not None and len(cb) != len(ca):
        raise ValueError(f"{who}: counts_a has {len(ca)} groups and counts_b {len(cb)}")
    if framed:
        if len(ca) != P:
            raise ValueError(f"{who}: counts must have one entry per image of the table ({P}), got {len(ca)}")
        t = frames.table_host
        return True, ca, cb, t["H"].astype(np.int64) * t["W"].astype(np.int64) // 32, 0
    return False, ca, cb, None, (int(a.H) * int(a.W) + 31) // 32


def _check_plan(who: str, plan, ca, cb, gw, nwords) -> None:
    if not isinstance(plan, OverlapPlan) or plan.tiles is None:
        raise ValueError(f"{who}: plan must be the OverlapPlan of mask_overlap_plan (made for a device)")
    words = gw if gw is not None else np.full(len(ca), nwords, np.int64)
    if (plan.self_form != (cb is None) or not np.array_equal(plan.counts_a, ca) or not np.array_equal(plan.counts_b, ca if cb is None else cb)
            or not np.array_equal(plan.group_words, words)):
        raise ValueError(f"{who}: the plan was made for other counts or another frame")


def mask_overlap_plan(a, b=None, counts_a=None, counts_b=None, frames=None, device=None) -> OverlapPlan:
    """The tables ``mask_overlap`` would make for these arguments, made once: tile table (host and device), workspace, offsets.
    ``mask_overlap(..., plan=plan)`` is then a pure enqueue of two kernels - no upload, no host work that depends on the planes -
    and can be captured into a graph and replayed on new plane contents.  ``device="cpu"``: the host tables only."""
    who = "mask_overlap_plan"
    framed, ca, cb, gw, nwords = _geometry(who, a, b, counts_a, counts_b, frames)
    tiles, offsets = plan_tiles(ca, cb, gw, nwords)
    words = gw if gw is not None else np.full(len(ca), nwords, np.int64)
    host = OverlapPlan(tiles, None, None, offsets, ca, ca if cb is None else cb, cb is None, words)
    if device is not None and torch.device(device).type == "cpu":
        return host
    dev = a.bits.device if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"{who}: the planes must live on the GPU")
    with torch.cuda.device(dev):
        t = torch.as_tensor(tiles.view(np.uint8).reshape(-1), device=dev) if len(tiles) else torch.empty(0, dtype=torch.uint8, device=dev)
        ws = torch.empty(max(int(lib.la3d_mask_overlap_workspace_bytes(len(tiles))) // 4, 1), dtype=torch.int32, device=dev)
    return host._replace(tiles=t, workspace=ws)


def mask_overlap(a, b=None, counts_a=None, counts_b=None, frames=None, iou=None, stream=None, plan=None) -> MaskOverlap:
    """Pairwise overlap of bit planes (C-ABI ``la3d_mask_overlap``): for every group g - an image - and every row i of ``a`` and j
    of ``b`` in it, ``inter = popcount(a_i & b_j)``, the planes' own areas, and with ``iou`` the ratio in float64:
    ``"iou"``: inter / (area_a + area_b - inter), ``"iom"``: inter / min(area_a, area_b), ``"ioa"``: inter / area_a; a zero
    denominator gives 0.0.  ``a``, ``b``: both ``MaskBits`` of one frame, or both ``FrameBits`` with ``frames`` - any packed object
    with the frame table the planes were laid out for (another table: ValueError before any device work); ``b=None`` is the SELF
    form (the square matrix of ``a`` against itself; only the tiles on and above the diagonal are computed).  ``counts_a`` /
    ``counts_b``: host sequences of ints, the rows of each group - the rows of a group are contiguous; None: one group holding
    every row (``MaskBits`` only; for ``FrameBits`` they are required, one entry per image of the table, group g IS image g).
    Mismatched frames, counts that do not sum to the rows, or unequal group numbers raise ValueError before any device work.
    Returns ``MaskOverlap``.  Two kernels, no atomics, no host synchronisation; ``plan``: the ``OverlapPlan`` of
    ``mask_overlap_plan`` for the same arguments - without it the tile table is planned and uploaded here (one small copy).  The
    padding bits of a plane count as mask and are zero by the packers' contract.  A ``FrameBits`` row whose image index is not its
    group's, whose offset is not a multiple of 4 or whose plane does not end inside its buffer is refused on the device: area -1,
    inter -1, iou NaN, never an exception."""
    who = "mask_overlap"
    if iou not in _KINDS:
        raise ValueError(f"{who}: iou must be None, 'iou', 'iom' or 'ioa', not {iou!r}")
    framed, ca, cb, gw, nwords = _geometry(who, a, b, counts_a, counts_b, frames)
    if plan is not None:
        _check_plan(who, plan, ca, cb, gw, nwords)
    self_form = b is None
    rows_a, rows_b = int(ca.sum()), int(ca.sum() if self_form else cb.sum())
    args = _lib.MaskOverlapArgs(struct_size=C.sizeof(_lib.MaskOverlapArgs), G=len(ca), kind=_KINDS[iou], rows_a=rows_a, rows_b=rows_b)
    if framed:
        dev = _on_gpu(frames.table, a.bits)
        if b is not None:
            _on_gpu(frames.table, b.bits)
        args.frames, args.P, args.H, args.W = frames.table.data_ptr(), len(ca), max(int(frames.H), 1), max(int(frames.W), 1)
        args.a_bits, args.a_offsets, args.a_words = a.bits.data_ptr(), a.offsets.data_ptr(), int(a.bits.numel())
        ai = a.image_index.to(device=dev, dtype=torch.int32).contiguous()
        bi = None if self_form else b.image_index.to(device=dev, dtype=torch.int32).contiguous()
        args.a_image_index = ai.data_ptr()
        if not self_form:
            args.b_bits, args.b_offsets, args.b_words, args.b_image_index = b.bits.data_ptr(), b.offsets.data_ptr(), int(b.bits.numel()), bi.data_ptr()
        held = (a.bits, a.offsets, ai, frames.table) + (() if self_form else (b.bits, b.offsets, bi))
    else:
        args.a_stride = _bits_stride(a.bits, rows_a, int(a.H), int(a.W))
        if not self_form:
            args.b_stride = _bits_stride(b.bits, rows_b, int(b.H), int(b.W))
            if b.bits.device != a.bits.device:
                raise ValueError(f"{who}: a and b live on different devices")
        dev = a.bits.device
        args.nwords, args.a_bits = nwords, a.bits.data_ptr()
        if not self_form:
            args.b_bits = b.bits.data_ptr()
        held = (a.bits,) + (() if self_form else (b.bits,))
    with torch.cuda.device(dev):
        if plan is None:
            plan = mask_overlap_plan(a, b, ca, cb, frames, device=dev)
        npairs = int(plan.offsets[-1])
        inter = torch.empty(npairs, dtype=torch.int32, device=dev)
        ratio = torch.empty(npairs, dtype=torch.float64, device=dev) if iou is not None else None
        area_a = torch.empty(rows_a, dtype=torch.int32, device=dev)
        area_b = area_a if self_form else torch.empty(rows_b, dtype=torch.int32, device=dev)
        args.tiles, args.ntiles, args.npairs = plan.tiles.data_ptr(), len(plan.tiles_host), npairs
        args.inter, args.area_a, args.area_b = inter.data_ptr(), area_a.data_ptr(), area_b.data_ptr()
        args.iou = None if ratio is None else ratio.data_ptr()
        args.workspace, args.stream = plan.workspace.data_ptr(), _stream(stream).value
        check(lib.la3d_mask_overlap(C.byref(args)), "la3d_mask_overlap")
    _record(stream, inter, ratio, area_a, area_b, plan.tiles, plan.workspace, *held)
    return MaskOverlap(inter, ratio, area_a, area_b, plan.offsets, plan.counts_a, plan.counts_b)


def mask_iou(a, b=None, counts_a=None, counts_b=None, frames=None, stream=None, plan=None) -> MaskOverlap:
    """``mask_overlap(..., iou="iou")``: the mask-level IoU matrix of every image - what ``assign.assign_overlap`` matches on the
    device (``matrix(g, "iou")``, negated, is what ``scipy.optimize.linear_sum_assignment`` takes, the way ``hungarian_matching``
    takes the box-level one: the same answer)."""
    return mask_overlap(a, b, counts_a=counts_a, counts_b=counts_b, frames=frames, iou="iou", stream=stream, plan=plan)


def mask_nms(bits, scores, iou_threshold: float = 0.5, counts=None, labels=None, kind: str = "iou", frames=None, overlap=None,
             stream=None) -> torch.Tensor:
    """Greedy mask NMS per image (C-ABI ``la3d_mask_nms`` on the self form of ``mask_overlap``) -> ``keep`` bool (B,) on the device.
    ``bits``: ``MaskBits``, or ``FrameBits`` with ``frames``; ``counts``: the rows of each image (None: one image; required for
    ``FrameBits``); ``scores``: (B,) floats, host or device.  Within each group the rows are visited by descending score, ties going
    to the lower row - the order is built on the device with stable sorts, nothing synchronises.  A kept row t suppresses a later
    row u iff ``labels`` is None or ``labels[t] == labels[u]``, and ``inter[t, u] > iou_threshold * den[t, u]`` with ``den > 0`` -
    den = ``area_t + area_u - inter`` for ``kind="iou"``, ``min(area_t, area_u)`` for ``kind="iom"`` (a nested mask goes whatever
    its size); the decision is a float64 multiply, not a division.  A row with a NaN score is never kept and suppresses nothing; so
    is a ``FrameBits`` row the device refuses.  ``overlap``: the ``MaskOverlap`` of ``mask_overlap(bits, counts_a=counts, ...)``
    (self form) to reuse.  What stays goes into ``fit_instances_bits`` (``bits.bits[keep]``)."""
    who = "mask_nms"
    if kind not in ("iou", "iom"):
        raise ValueError(f"{who}: kind must be 'iou' or 'iom', not {kind!r}")
    if isinstance(iou_threshold, bool) or not isinstance(iou_threshold, (int, float, np.integer, np.floating)) or np.isnan(float(iou_threshold)):
        raise ValueError(f"{who}: iou_threshold must be a number, not {iou_threshold!r}")
    _, ca, _, gw, nwords = _geometry(who, bits, None, counts, None, frames)
    B, G = int(ca.sum()), len(ca)
    for name, x in (("scores", scores), ("labels", labels)):
        if x is not None and tuple(x.shape if isinstance(x, torch.Tensor) else np.shape(x)) != (B,):
            raise ValueError(f"{who}: {name} must hold one value per row ({B})")
    if overlap is not None:
        if not isinstance(overlap, MaskOverlap) or not np.array_equal(overlap.counts_a, ca) or not np.array_equal(overlap.counts_b, ca) \
                or overlap.area_a.data_ptr() != overlap.area_b.data_ptr():
            raise ValueError(f"{who}: overlap must be the self form of mask_overlap for the same planes and counts")
    else:
        overlap = mask_overlap(bits, counts_a=ca, frames=frames, stream=stream)
    dev = overlap.inter.device
    with torch.cuda.device(dev):
        s = scores.to(dev) if isinstance(scores, torch.Tensor) else torch.as_tensor(np.asarray(scores, np.float64), device=dev)
        if not s.is_floating_point():
            s = s.to(torch.float64)
        lab = None if labels is None else (labels.to(device=dev, dtype=torch.int32).contiguous() if isinstance(labels, torch.Tensor)
                                           else torch.as_tensor(np.asarray(labels).astype(np.int32), device=dev))
        rows = np.zeros(G + 1, np.int32)
        np.cumsum(ca, out=rows[1:])
        gid, row_offsets, offsets = _upload_many([(np.repeat(np.arange(G, dtype=np.int64), ca), torch.int64), (rows, torch.int32),
                                                  (overlap.offsets, torch.int64)], dev)
        nan = torch.isnan(s)
        by_score = torch.sort(torch.where(nan, torch.full_like(s, float("-inf")), s), descending=True, stable=True).indices
        order = by_score[torch.sort(gid[by_score], stable=True).indices]
        order = torch.where(nan[order], torch.full_like(order, -1), order).to(torch.int32)
        keep = torch.empty(B, dtype=torch.uint8, device=dev)
        args = _lib.MaskNmsArgs(struct_size=C.sizeof(_lib.MaskNmsArgs), G=G, kind=_KINDS[kind], B=B, inter=overlap.inter.data_ptr(),
                                area=overlap.area_a.data_ptr(), offsets=offsets.data_ptr(), row_offsets=row_offsets.data_ptr(),
                                order=order.data_ptr(), labels=None if lab is None else lab.data_ptr(), thr=float(iou_threshold),
                                keep=keep.data_ptr(), stream=_stream(stream).value)
        check(lib.la3d_mask_nms(C.byref(args)), "la3d_mask_nms")
    _record(stream, overlap.inter, overlap.area_a, offsets, row_offsets, order, lab, keep)
    return keep.view(torch.bool)
