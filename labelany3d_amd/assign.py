"""Batched assignment on the device (include/la3d.h "assignment on the device"): the step that reads the matrices of
``mask_overlap`` / ``mask_iou`` (bit planes) and of the box-level IoU - the Hungarian matching of the reference's stage 8
(``hungarian_matching``, src/tools/combine_results.py:126-144) - for every image of a call at once, without a copy to the host.
The arithmetic is ``scipy.optimize.linear_sum_assignment`` (SciPy 1.15) step for step, ties included: ``Assignment.pairs(g)`` is
SciPy's ``(rows, cols)`` of group g's matrix, exactly."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from ._device import _as_dev, _dev, _record, _stream, _upload_many
from .overlap import MaskOverlap, _counts, mask_overlap

MAX_N = _lib.ASSIGN_MAX_N
"""The most rows or columns a group may have (``LA3D_ASSIGN_MAX_N``); a larger group gets status 3 and no assignment."""

_MESSAGES = {_lib.ASSIGN_INVALID: "matrix contains invalid numeric entries", _lib.ASSIGN_INFEASIBLE: "cost matrix is infeasible"}


class AssignPlan(NamedTuple):
    """The tables of one assignment call shape on the device (``assign_plan``): with them ``assign_batch`` / ``assign_overlap`` are a
    pure enqueue of one kernel - no upload - and can be captured into a graph."""
    offsets_host: np.ndarray
    counts_a: np.ndarray
    counts_b: np.ndarray
    offsets: torch.Tensor
    row_offsets_a: torch.Tensor
    row_offsets_b: torch.Tensor
    row_base: torch.Tensor      # int64 (rows of A,): where the row's part of its group's matrix begins in the flat buffer
    col_base: torch.Tensor      # int64 (rows of A,): the first row of B of the row's group


class Assignment:
    """What the assignment calls return.  On the device: ``col_of_row`` int32 (rows of A,) - the column a row is matched with, counted
    within its group, -1 if none -, ``row_of_col`` int32 (rows of B,) likewise, ``status`` int32 (G,): 0 assigned, 1 an invalid entry
    (NaN, or -inf after the sign of ``maximize``), 2 infeasible, 3 more than ``MAX_N`` rows or columns, 4 broken tables.  With status
    1 - 3 every row and column of the group is -1.  On the host: ``counts_a`` / ``counts_b`` int32 (G,).  ``value`` (``match_masks``,
    ``match_boxes``): float64 (rows of A,) on the device, the matched pair's ratio, NaN where unmatched."""

    def __init__(self, col_of_row, row_of_col, status, counts_a, counts_b, value=None):
        self.col_of_row, self.row_of_col, self.status = col_of_row, row_of_col, status
        self.counts_a, self.counts_b, self.value = counts_a, counts_b, value
        self._host = self._first = None

    def host(self):
        """``(col_of_row, row_of_col, status)`` as NumPy - one copy back for the whole call, made once.  It synchronises."""
        if self._host is None:
            packed = torch.cat([self.col_of_row, self.row_of_col, self.status]).cpu().numpy()
            na, nb = int(self.col_of_row.numel()), int(self.row_of_col.numel())
            self._host = packed[:na], packed[na:na + nb], packed[na + nb:]
        return self._host

    def pairs(self, g: int):
        """``(rows, cols)`` of group ``g`` as NumPy int64, rows ascending: what ``scipy.optimize.linear_sum_assignment`` returns for
        the group's matrix (empty for a group whose status is not 0).  It synchronises."""
        g = int(g)
        if not 0 <= g < len(self.counts_a):
            raise ValueError(f"pairs: group {g} outside [0, {len(self.counts_a)})")
        if self._first is None:
            self._first = np.concatenate([[0], np.cumsum(self.counts_a, dtype=np.int64)])
        a0 = int(self._first[g])
        col = self.host()[0][a0:a0 + int(self.counts_a[g])]
        rows = np.flatnonzero(col >= 0)
        return rows.astype(np.int64), col[rows].astype(np.int64)

    def raise_for_status(self) -> None:
        """ValueError for the first group whose status is not 0: SciPy's message where SciPy raises one.  It synchronises."""
        st = self.host()[2]
        for g in np.flatnonzero(st != 0):
            s = int(st[g])
            if s in _MESSAGES:
                raise ValueError(_MESSAGES[s])
            if s == _lib.ASSIGN_TOO_LARGE:
                raise ValueError(f"group {int(g)} has more than {MAX_N} rows or columns ({int(self.counts_a[g])} x {int(self.counts_b[g])})")
            raise ValueError(f"group {int(g)}: the tables of the call are broken (status {s})")


def _tables(who: str, offsets, counts_a, counts_b, ncost: int):
    """The host tables of a call, checked: counts (G,), offsets (G + 1,) with every matrix inside the cost buffer."""
    if counts_a is None or counts_b is None:
        raise ValueError(f"{who}: counts_a and counts_b are required")
    ca = _counts(who, "counts_a", counts_a, int(np.sum(np.asarray(counts_a, dtype=np.int64))) if _plain(counts_a) else 0)
    cb = _counts(who, "counts_b", counts_b, int(np.sum(np.asarray(counts_b, dtype=np.int64))) if _plain(counts_b) else 0)
    if len(ca) != len(cb):
        raise ValueError(f"{who}: counts_a has {len(ca)} groups and counts_b {len(cb)}")
    G = len(ca)
    sizes = ca.astype(np.int64) * cb.astype(np.int64)
    if offsets is None:
        off = np.zeros(G + 1, np.int64)
        np.cumsum(sizes, out=off[1:])
    else:
        if isinstance(offsets, torch.Tensor):
            raise ValueError(f"{who}: offsets must be a host sequence of ints")
        off = np.asarray(offsets)
        if off.ndim != 1 or len(off) != G + 1 or not np.issubdtype(off.dtype, np.integer):
            raise ValueError(f"{who}: offsets must hold G + 1 = {G + 1} ints")
        off = off.astype(np.int64)
    if G and (int(off[:-1].min()) < 0 or int((off[:-1] + sizes).max()) > ncost):
        raise ValueError(f"{who}: a group's matrix lies outside the {ncost} elements of cost")
    if int(ca.sum()) > 0x7fffffff or int(cb.sum()) > 0x7fffffff:
        raise ValueError(f"{who}: more than 2^31 - 1 rows in one call")
    return ca, cb, off


def _plain(x) -> bool:
    try:
        a = np.asarray(list(x) if not isinstance(x, np.ndarray) else x)
    except TypeError:
        return False
    return not isinstance(x, torch.Tensor) and a.ndim == 1 and (a.size == 0 or np.issubdtype(a.dtype, np.integer))


def _row_offsets(c: np.ndarray) -> np.ndarray:
    r = np.zeros(len(c) + 1, np.int32)
    np.cumsum(c, out=r[1:])
    return r


def assign_plan(offsets, counts_a, counts_b, ncost: Optional[int] = None, device=None) -> AssignPlan:
    """The device tables of an assignment call, uploaded once (one copy): ``offsets`` host ints (G + 1,) - None: the matrices follow
    each other -, ``counts_a`` / ``counts_b`` the rows and columns of each group.  ``ncost``: the elements of the cost buffer the plan
    will be used with (None: the end of the last matrix)."""
    who = "assign_plan"
    ca, cb, off = _tables(who, offsets, counts_a, counts_b, 1 << 62 if ncost is None else int(ncost))
    dev = _dev(device)
    if dev.type != "cuda":
        raise ValueError(f"{who}: the tables must live on the GPU")
    with torch.cuda.device(dev):
        fa, fb = _row_offsets(ca), _row_offsets(cb)
        reps = ca.astype(np.int64)
        local = np.arange(int(fa[-1]), dtype=np.int64) - np.repeat(fa[:-1].astype(np.int64), reps)
        row_base = np.repeat(off[:-1], reps) + local * np.repeat(cb.astype(np.int64), reps)
        o, ra, rb, base, cbase = _upload_many([(off, torch.int64), (fa, torch.int32), (fb, torch.int32), (row_base, torch.int64),
                                               (np.repeat(fb[:-1].astype(np.int64), reps), torch.int64)], dev)
    return AssignPlan(off, ca, cb, o, ra, rb, base, cbase)


def _launch(cost: torch.Tensor, plan: AssignPlan, maximize: bool, stream) -> Assignment:
    """One ``la3d_assign`` call on a flat device buffer with the plan's tables."""
    dev = cost.device
    G, rows_a, rows_b = len(plan.counts_a), int(plan.counts_a.sum()), int(plan.counts_b.sum())
    off, ra, rb = plan.offsets, plan.row_offsets_a, plan.row_offsets_b
    with torch.cuda.device(dev):
        col = torch.empty(rows_a, dtype=torch.int32, device=dev)
        row = torch.empty(rows_b, dtype=torch.int32, device=dev)
        status = torch.empty(G, dtype=torch.int32, device=dev)
        args = _lib.AssignArgs(struct_size=C.sizeof(_lib.AssignArgs), G=G, cost=cost.data_ptr() if cost.numel() else None,
                               cost_dtype=_lib.ASSIGN_I32 if cost.dtype == torch.int32 else _lib.ASSIGN_F64, ncost=int(cost.numel()),
                               offsets=off.data_ptr(), row_offsets_a=ra.data_ptr(), row_offsets_b=rb.data_ptr(), rows_a=rows_a, rows_b=rows_b,
                               maximize=1 if maximize else 0, col_of_row=col.data_ptr() if rows_a else None,
                               row_of_col=row.data_ptr() if rows_b else None, status=status.data_ptr() if G else None,
                               stream=_stream(stream).value)
        check(lib.la3d_assign(C.byref(args)), "la3d_assign")
    _record(stream, cost, off, ra, rb, col, row, status)
    return Assignment(col, row, status, plan.counts_a, plan.counts_b)


def _check_cost(who: str, cost):
    if isinstance(cost, torch.Tensor):
        if cost.dtype not in (torch.float64, torch.int32):
            raise ValueError(f"{who}: cost must be float64 or int32, not {cost.dtype}")
        if not cost.is_cuda:
            raise ValueError(f"{who}: a cost tensor must live on the GPU (a NumPy array is uploaded)")
        return cost
    a = np.asarray(cost)
    if a.dtype not in (np.float64, np.int32):
        raise ValueError(f"{who}: cost must be float64 or int32, not {a.dtype}")
    return a


def _flag(who: str, name: str, x) -> bool:
    if not isinstance(x, (bool, np.bool_)):
        raise ValueError(f"{who}: {name} must be True or False, not {x!r}")
    return bool(x)


def _use_plan(who: str, plan, ca, cb, off) -> None:
    if not isinstance(plan, AssignPlan):
        raise ValueError(f"{who}: plan must be the AssignPlan of assign_plan")
    if not (np.array_equal(plan.counts_a, ca) and np.array_equal(plan.counts_b, cb) and np.array_equal(plan.offsets_host, off)):
        raise ValueError(f"{who}: the plan was made for other counts or offsets")


def assign_batch(cost, offsets, counts_a, counts_b, maximize: bool = False, stream=None, plan: Optional[AssignPlan] = None) -> Assignment:
    """The linear sum assignment of every group of a flat cost buffer (C-ABI ``la3d_assign``): group g's matrix is the
    ``counts_a[g] x counts_b[g]`` elements at ``cost[offsets[g]:]``, row-major.  ``cost``: float64 or int32, a device tensor (read
    where it lies) or a NumPy array; ``offsets``: host ints (G + 1,), None: the matrices follow each other; ``maximize``: as SciPy's.
    One kernel, one wave per group, no host synchronisation; without ``plan`` (``assign_plan``) the small tables are uploaded
    here in one copy.  At most ``MAX_N`` rows and columns per group (status 3 beyond).  Returns ``Assignment``."""
    who = "assign_batch"
    cost = _check_cost(who, cost)
    maximize = _flag(who, "maximize", maximize)
    ca, cb, off = _tables(who, offsets, counts_a, counts_b, int(cost.size if isinstance(cost, np.ndarray) else cost.numel()))
    if plan is not None:
        _use_plan(who, plan, ca, cb, off)
    dev = cost.device if isinstance(cost, torch.Tensor) else (plan.offsets.device if plan is not None else _dev())
    with torch.cuda.device(dev):
        flat = _as_dev(cost, torch.float64 if cost.dtype in (torch.float64, np.float64) else torch.int32, dev).reshape(-1)
        if plan is None:
            plan = assign_plan(off, ca, cb, device=dev)
    return _launch(flat, plan, maximize, stream)


def assign_overlap(overlap, what: str = "iou", maximize: bool = True, stream=None, plan: Optional[AssignPlan] = None) -> Assignment:
    """The assignment straight on a ``MaskOverlap``: ``what`` = "iou" matches by its ratio (float64), "inter" by the intersection
    counts (int32, exact).  ``maximize`` defaults to True - the most overlap.  A refused ``FrameBits`` row (iou NaN) makes its group
    status 1, as SciPy raises; with "inter" its -1 simply loses."""
    who = "assign_overlap"
    if not isinstance(overlap, MaskOverlap):
        raise ValueError(f"{who}: overlap must be the MaskOverlap of mask_overlap / mask_iou")
    if what not in ("iou", "inter"):
        raise ValueError(f"{who}: what must be 'iou' or 'inter', not {what!r}")
    maximize = _flag(who, "maximize", maximize)
    cost = overlap.inter if what == "inter" else overlap.iou
    if cost is None:
        raise ValueError(f"{who}: this overlap was computed without iou")
    if plan is not None:
        _use_plan(who, plan, overlap.counts_a, overlap.counts_b, overlap.offsets)
    else:
        plan = assign_plan(overlap.offsets, overlap.counts_a, overlap.counts_b, ncost=int(cost.numel()), device=cost.device)
    return _launch(cost, plan, maximize, stream)


def _matched_value(a: Assignment, ratio: torch.Tensor, plan: AssignPlan, min_value) -> Assignment:
    """``value`` of every row of A from the flat ratio buffer, and the ``min_value`` gate (a few torch ops on the current stream)."""
    rows_a, rows_b = int(a.col_of_row.numel()), int(a.row_of_col.numel())
    nan = torch.full((rows_a,), float("nan"), dtype=torch.float64, device=a.col_of_row.device)
    if rows_a == 0 or int(ratio.numel()) == 0:
        a.value = nan
        return a
    col = a.col_of_row.to(torch.int64)
    has = col >= 0
    col = col.clamp(min=0)
    value = torch.where(has, ratio[(plan.row_base + col).clamp(max=int(ratio.numel()) - 1)], nan)
    if min_value is not None:
        keep = has & (value >= float(min_value))
        # (the dropped pairs' columns, without a synchronising nonzero: every other row aims at one spare slot behind the columns)
        spare = torch.cat([a.row_of_col, a.row_of_col.new_zeros(1)])
        a.row_of_col = spare.index_fill(0, torch.where(has & ~keep, plan.col_base + col, torch.full_like(col, rows_b)), -1)[:rows_b]
        a.col_of_row = torch.where(keep, a.col_of_row, torch.full_like(a.col_of_row, -1))
        value = torch.where(keep, value, nan)
    a.value = value
    return a


def match_masks(a, b, counts_a=None, counts_b=None, frames=None, kind: str = "iou", min_value=None, plan=None, stream=None) -> Assignment:
    """Match the masks of ``a`` with those of ``b``, image by image: ``mask_overlap(a, b, ..., iou=kind)`` and the assignment that
    maximises the ratio, on one stream and without a synchronisation.  ``a``, ``b``: both ``MaskBits``, or both ``FrameBits`` with
    ``frames``; ``kind``: "iou", "iom" or "ioa"; ``plan``: the ``OverlapPlan`` of ``mask_overlap_plan``.  Returns the ``Assignment``
    with ``value`` - float64 per row of ``a``: the matched pair's ratio, NaN where unmatched.  ``min_value``: a pair whose value is
    not ``>= min_value`` becomes unmatched on both sides (SciPy matches every row of the smaller side, pairs without overlap too)."""
    who = "match_masks"
    if kind not in ("iou", "iom", "ioa"):
        raise ValueError(f"{who}: kind must be 'iou', 'iom' or 'ioa', not {kind!r}")
    if b is None:
        raise ValueError(f"{who}: b is required (masks are matched between two sets)")
    if min_value is not None and (isinstance(min_value, bool) or not isinstance(min_value, (int, float, np.integer, np.floating))
                                  or np.isnan(float(min_value))):
        raise ValueError(f"{who}: min_value must be a number or None, not {min_value!r}")
    try:
        ov = mask_overlap(a, b, counts_a=counts_a, counts_b=counts_b, frames=frames, iou=kind, stream=stream, plan=plan)
    except ValueError as e:
        raise ValueError(str(e).replace("mask_overlap:", f"{who}:", 1)) from None
    dev = ov.inter.device
    with torch.cuda.device(dev):
        ap = assign_plan(ov.offsets, ov.counts_a, ov.counts_b, ncost=int(ov.iou.numel()), device=dev)
        out = _launch(ov.iou, ap, True, stream)
        s = torch.cuda.current_stream() if stream is None else stream
        with torch.cuda.stream(s):
            out = _matched_value(out, ov.iou, ap, min_value)
    return out


class BoxIou(NamedTuple):
    """What ``iou2d_groups`` returns: ``iou`` float64, flat, on the device - group g's (n0_g, n1_g) matrix at ``offsets[g]``,
    row-major -, and the plan that holds the tables."""
    iou: torch.Tensor
    plan: AssignPlan

    def matrix(self, g: int) -> torch.Tensor:
        g = int(g)
        o = self.plan.offsets_host
        return self.iou[int(o[g]):int(o[g + 1])].view(int(self.plan.counts_a[g]), int(self.plan.counts_b[g]))


def _boxes(who: str, name: str, x):
    shape = tuple(x.shape) if isinstance(x, torch.Tensor) else np.shape(x)
    if len(shape) == 2 and shape[1] == 4:
        return shape[0]
    if len(shape) == 1 and shape[0] == 0:
        return 0
    raise ValueError(f"{who}: {name} must be (n, 4) xyxy boxes, not {shape}")


def iou2d_groups(boxes0, boxes1, counts0=None, counts1=None, stream=None, _who: str = "iou2d_groups") -> BoxIou:
    """``iou2d_matrix`` for every group of a call in one launch (C-ABI ``la3d_iou_matrix_groups``): ``boxes0`` (n0, 4), ``boxes1``
    (n1, 4) xyxy, the rows of a group contiguous; ``counts0`` / ``counts1``: the boxes of each group (None: one group).  Every group's
    values are bit-identical to ``iou2d_matrix`` on that group."""
    who = _who
    n0, n1 = _boxes(who, "boxes0", boxes0), _boxes(who, "boxes1", boxes1)
    c0 = _counts(who, "counts0", [n0] if counts0 is None else counts0, n0)
    c1 = _counts(who, "counts1", [n1] if counts1 is None else counts1, n1)
    if len(c0) != len(c1):
        raise ValueError(f"{who}: counts0 has {len(c0)} groups and counts1 {len(c1)}")
    _, _, off = _tables(who, None, c0, c1, 1 << 62)
    dev = boxes0.device if isinstance(boxes0, torch.Tensor) and boxes0.is_cuda else _dev()
    with torch.cuda.device(dev):
        plan = assign_plan(off, c0, c1, device=dev)
        a, b = _as_dev(boxes0, torch.float64, dev).reshape(-1, 4), _as_dev(boxes1, torch.float64, dev).reshape(-1, 4)
        npairs = int(off[-1])
        out = torch.empty(npairs, dtype=torch.float64, device=dev)
        args = _lib.IouGroupsArgs(struct_size=C.sizeof(_lib.IouGroupsArgs), G=len(c0), boxes_a=a.data_ptr() if n0 else None,
                                  boxes_b=b.data_ptr() if n1 else None, rows_a=n0, rows_b=n1, row_offsets_a=plan.row_offsets_a.data_ptr(),
                                  row_offsets_b=plan.row_offsets_b.data_ptr(), offsets=plan.offsets.data_ptr(), npairs=npairs,
                                  out=out.data_ptr() if npairs else None, stream=_stream(stream).value)
        check(lib.la3d_iou_matrix_groups(C.byref(args)), "la3d_iou_matrix_groups")
    _record(stream, a, b, out, plan.offsets, plan.row_offsets_a, plan.row_offsets_b)
    return BoxIou(out, plan)


def match_boxes(boxes0, boxes1, counts0=None, counts1=None, stream=None) -> Assignment:
    """Match the xyxy boxes of ``boxes0`` with those of ``boxes1``, group by group (an image, a scene): the grouped box IoU and the
    assignment that maximises it, two kernels on one stream, no synchronisation.  Returns the ``Assignment`` with ``value`` = the
    matched pair's IoU.  With one group, ``pairs(0)`` and ``value`` are what ``hungarian_matching(boxes0, boxes1)`` lists."""
    who = "match_boxes"
    iou = iou2d_groups(boxes0, boxes1, counts0, counts1, stream=stream, _who=who)
    dev = iou.iou.device
    with torch.cuda.device(dev):
        out = _launch(iou.iou, iou.plan, True, stream)
        s = torch.cuda.current_stream() if stream is None else stream
        with torch.cuda.stream(s):
            out = _matched_value(out, iou.iou, iou.plan, None)
    return out
