"""Masked depth statistics next to the box fit: the data-parallel parts of the reference's two depth
alignment helpers, on the MI355X.

* ``align_depth`` — drop-in for reference src/batch_scripts/depth.py:52-92 (stage 1: MoGe depth aligned to DepthPro's
  metric scale).  The valid-pixel selection / compaction (:67-78) and the prediction scatter (:82-90) are HIP kernels
  (``la3d_align_select`` / ``la3d_align_apply``); the estimator in between is the reference's own third-party call,
  ``sklearn.linear_model.RANSACRegressor(LinearRegression(fit_intercept=False), min_samples=...)``, fed the same samples in
  the same (row-major) order and drawing from the same global NumPy stream, so a seeded run reproduces the reference.
* ``depth_match_transform`` — the arithmetic of ``align_to_depth_match`` (src/util.py:464-494) after its renderer call:
  overlap = mask & render alpha; scale = median(depth_map[overlap] / depth_render[overlap]) (``la3d_masked_ratio_median``,
  exact radix select on the GPU); transform = [inv(R[:3,:3]) * scale | T * scale].
* ``align_depth_batch`` - ``align_depth`` for a stack of frames with the estimator on the GPU as well (``ransac_scale_batch``, C-ABI
  ``la3d_align_ransac_batch``: scikit-learn's RANSAC loop for the one-parameter model, all trials judged in one sweep): select -> fit
  -> apply without a host synchronisation.  The subsets are drawn on the device from a seed (not NumPy's stream), or given.
* ``ground_planes`` - the ``ground`` vector of the fit entries from the depth itself (include/la3d.h "ground plane: RANSAC plane fit"):
  ``plane_select_batch`` (grid samples, back-projected) -> ``plane_ransac_batch`` (batched RANSAC plane fit, the same device draw with
  m = 3), for a stack of images of one size, without a host synchronisation; ``PlaneFit.for_instances`` hands the planes to a fit.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from ._device import _as_dev, _dev, _ptr, _record, _stream
from ._lib import AlignRansacArgs, PlaneRansacArgs, PlaneSelectArgs, check, lib
from .bits import MaskBits


def align_select(relative_depth, metric_depth, mask=None, max_valid_depth: float = 400.0, device=None, stream=None):
    """``relative[valid], metric[valid]`` with ``valid = ~isinf(relative) & (metric < max_valid_depth) [& mask]`` in row-major
    order (reference depth.py:67-78), on the GPU.  Returns two float32 tensors of equal length."""
    dev = _dev(device)
    rel = _as_dev(relative_depth, torch.float32, dev).reshape(-1)
    met = _as_dev(metric_depth, torch.float32, dev).reshape(-1)
    if rel.numel() != met.numel():
        raise ValueError("relative_depth and metric_depth differ in size")
    m = None if mask is None else _as_dev(mask, torch.uint8, dev).reshape(-1)
    n = rel.numel()
    ro, mo = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.la3d_align_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.la3d_align_select(_ptr(rel), _ptr(met), _ptr(m), n, float(max_valid_depth), _ptr(ro), _ptr(mo), _ptr(cnt),
                                    _ptr(ws), _stream(stream)), "la3d_align_select")
    k = int(cnt.item())
    return ro[:k], mo[:k]


def align_select_batch(relative_depth, metric_depth, mask=None, max_valid_depth: float = 400.0, device=None, stream=None):
    """``align_select`` for a stack of P frames in one call (C-ABI ``la3d_align_select_batch``; the reference loops over images,
    src/batch_scripts/depth.py:138-160): ``relative_depth`` / ``metric_depth`` (P,H,W) [``mask`` (P,H,W)] ->
    ``(rel_sel (P,n), met_sel (P,n), counts (P,) int64)``, all on the GPU and without any host synchronisation; frame p's selection
    is ``rel_sel[p, :counts[p]]`` in row-major order."""
    dev = _dev(device)
    rel = _as_dev(relative_depth, torch.float32, dev)
    met = _as_dev(metric_depth, torch.float32, dev)
    if rel.dim() < 2 or rel.shape != met.shape:
        raise ValueError("relative_depth and metric_depth must be stacks of equal shape (P, ...)")
    P = rel.shape[0]
    rel, met = rel.reshape(P, -1), met.reshape(P, -1)
    n = rel.shape[1]
    m = None
    if mask is not None:
        m = _as_dev(mask, torch.uint8, dev).reshape(P, -1)
        if m.shape != rel.shape:
            raise ValueError("mask must have the shape of the depth stack")
    ro, mo = torch.empty((P, n), dtype=torch.float32, device=dev), torch.empty((P, n), dtype=torch.float32, device=dev)
    cnt = torch.zeros(P, dtype=torch.int64, device=dev)
    ws = torch.empty(max(P, 1) * int(lib.la3d_align_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.la3d_align_select_batch(_ptr(rel), _ptr(met), _ptr(m), P, n, float(max_valid_depth), _ptr(ro), _ptr(mo), _ptr(cnt),
                                          _ptr(ws), _stream(stream)), "la3d_align_select_batch")
    return ro, mo, cnt


def align_apply(relative_depth, coef, intercept=0.0, mask=None, fill: float = 10000.0, device=None, stream=None):
    """``depth = full(fill); depth[sel] = relative[sel] * coef + intercept`` in float32, ``sel`` = mask if given else
    ``~isinf(relative)`` (reference depth.py:82-90).  Returns a float32 tensor shaped like ``relative_depth``."""
    dev = _dev(device)
    rel = _as_dev(relative_depth, torch.float32, dev)
    m = None if mask is None else _as_dev(mask, torch.uint8, dev)
    out = torch.empty_like(rel)
    with torch.cuda.device(dev):
        check(lib.la3d_align_apply(_ptr(rel), _ptr(m), rel.numel(), float(np.float32(coef)), float(np.float32(intercept)), float(fill),
                                   _ptr(out), _stream(stream)), "la3d_align_apply")
    return out


def align_depth(relative_depth, metric_depth, mask=None, min_samples=0.2, max_valid_depth=400.0):
    """Drop-in for the reference's ``align_depth`` (src/batch_scripts/depth.py:52-92): same arguments, same return (a float32
    array shaped like the input; ``metric_depth`` itself when nothing is valid or the fit fails), same printed messages,
    same consumption of the global NumPy stream by RANSAC."""
    from sklearn.linear_model import LinearRegression, RANSACRegressor   # the reference's estimator (depth.py:30, :66)

    regressor = RANSACRegressor(estimator=LinearRegression(fit_intercept=False), min_samples=min_samples)
    rel_sel, met_sel = align_select(relative_depth, metric_depth, mask, max_valid_depth)
    if rel_sel.numel() == 0:
        print("Warning: No valid points for alignment. Returning metric depth.")
        return metric_depth
    try:
        regressor.fit(rel_sel.cpu().numpy().reshape(-1, 1), met_sel.cpu().numpy().reshape(-1, 1))
    except Exception as e:  # noqa: BLE001 - the reference catches everything here (:76-78)
        print(f"Error fitting RANSACRegressor: {e}, using metric depth directly")
        return metric_depth
    est = regressor.estimator_
    coef = np.asarray(est.coef_, dtype=np.float32).reshape(-1)[0]
    intercept = np.asarray(est.intercept_, dtype=np.float32).reshape(-1)[0]
    out = align_apply(relative_depth, coef, intercept, mask)
    if isinstance(relative_depth, torch.Tensor):
        return out
    return out.cpu().numpy().reshape(np.asarray(relative_depth).shape)


class RansacScale(NamedTuple):
    """Result of ``ransac_scale_batch``, device tensors of length P: ``coef`` float32 (NaN where status != 0); ``n_inliers``,
    ``n_trials``, ``best_trial`` (-1 where status != 0) and ``status`` int32 - 0 fitted, 1 no valid sample, 2 the fit failed (the two
    cases for which the reference's ``align_depth`` prints a message and returns the metric depth)."""
    coef: torch.Tensor
    n_inliers: torch.Tensor
    n_trials: torch.Tensor
    best_trial: torch.Tensor
    status: torch.Tensor


def ransac_scale_batch(rel_sel, met_sel, counts, min_samples=0.2, max_trials: int = 100, subsets=None, seed: int = 0, stream=None,
                       stop_probability: float = 0.99) -> RansacScale:
    """scikit-learn's ``RANSACRegressor(LinearRegression(fit_intercept=False), min_samples=...)`` for P frames in one call on the GPU
    (C-ABI ``la3d_align_ransac_batch``; semantics in include/la3d.h): ``rel_sel`` / ``met_sel`` (P,n) float32 and ``counts`` (P,)
    int64 as ``align_select_batch`` leaves them.  ``subsets``: int32 (P, max_trials, m_cap) - trial t of frame p uses the first
    m = ceil(min_samples * counts[p]) entries of its row (a seeded scikit-learn draw made on the host) -, or None: drawn on the device
    from ``seed`` (counter-based, m distinct indices per trial; NOT NumPy's stream - ``ransac_subsets`` exports it).  No host
    synchronisation; returns a ``RansacScale`` of device tensors."""
    dev = rel_sel.device if isinstance(rel_sel, torch.Tensor) and rel_sel.is_cuda else _dev(None)
    x = _as_dev(rel_sel, torch.float32, dev)
    y = _as_dev(met_sel, torch.float32, dev)
    if x.dim() != 2 or x.shape != y.shape:
        raise ValueError("rel_sel and met_sel must be (P, n) stacks of equal shape")
    P, n = x.shape
    cnt = _as_dev(counts, torch.int64, dev).reshape(-1)
    if cnt.numel() != P:
        raise ValueError("counts must hold one entry per frame")
    sub, m_cap = None, 0
    if subsets is not None:
        sub = _as_dev(subsets, torch.int32, dev)
        if sub.dim() != 3 or sub.shape[0] != P or sub.shape[1] != int(max_trials):
            raise ValueError("subsets must be (P, max_trials, m_cap)")
        m_cap = int(sub.shape[2])
    coef = torch.empty(P, dtype=torch.float32, device=dev)
    ints = torch.empty((4, P), dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.la3d_align_ransac_workspace_bytes(P, n, int(max_trials))), dtype=torch.uint8, device=dev)
    a = AlignRansacArgs(struct_size=C.sizeof(AlignRansacArgs), P=P, n=n, relative_sel=x.data_ptr(), metric_sel=y.data_ptr(),
                        counts=cnt.data_ptr(), min_samples=float(min_samples), stop_probability=float(stop_probability),
                        max_trials=int(max_trials), m_cap=m_cap, subsets=None if sub is None else sub.data_ptr(),
                        seed=int(seed) & 0xFFFFFFFFFFFFFFFF, coef=coef.data_ptr(), n_inliers=ints[0].data_ptr(),
                        n_trials=ints[1].data_ptr(), best_trial=ints[2].data_ptr(), status=ints[3].data_ptr(),
                        workspace=ws.data_ptr())
    with torch.cuda.device(dev):
        a.stream = _stream(stream).value
        check(lib.la3d_align_ransac_batch(C.byref(a)), "la3d_align_ransac_batch")
    _record(stream, x, y, cnt, sub, coef, ints, ws)
    return RansacScale(coef, ints[0], ints[1], ints[2], ints[3])


def ransac_subsets(counts, min_samples=0.2, max_trials: int = 100, seed: int = 0, device=None, stream=None):
    """The subsets the device draw of ``ransac_scale_batch(..., subsets=None, seed=seed)`` uses (C-ABI ``la3d_align_ransac_subsets``),
    for reproducing or auditing a fit: int32 (P, max_trials, m_cap) on the GPU with m_cap the largest subset size of the batch; row
    (p, t) holds m_p distinct indices into frame p's samples, then -1.  Reads ``counts`` back once to size the result."""
    dev = counts.device if isinstance(counts, torch.Tensor) and counts.is_cuda else _dev(device)
    cnt = _as_dev(counts, torch.int64, dev).reshape(-1)
    P = cnt.numel()
    n_top = int(cnt.max().item()) if P else 0
    if 0 < float(min_samples) < 1:
        m_cap = int(np.ceil(np.float64(min_samples) * np.float64(max(n_top, 0))))
    else:
        m_cap = int(min_samples)
    m_cap = max(m_cap, 1)
    out = torch.empty((P, int(max_trials), m_cap), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.la3d_align_ransac_subsets(_ptr(cnt), P, float(min_samples), int(max_trials), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out),
                                            m_cap, _stream(stream)), "la3d_align_ransac_subsets")
    _record(stream, cnt, out)
    return out


def align_depth_batch(relative_depth, metric_depth, mask=None, min_samples=0.2, max_valid_depth: float = 400.0, subsets=None,
                      seed: int = 0, stream=None, max_trials: int = 100):
    """``align_depth`` (reference src/batch_scripts/depth.py:52-92) for a stack of P frames, every step on the GPU: ``relative_depth``
    / ``metric_depth`` (P,H,W) [``mask`` (P,H,W)] -> ``(aligned (P,H,W) float32, RansacScale)``.  Chains ``align_select_batch`` ->
    ``ransac_scale_batch`` -> the prediction scatter (C-ABI ``la3d_align_apply_batch``) without ``.item()``, ``.cpu()`` or a loop over
    frames.  A frame whose status is not 0 comes back as its metric depth - what the reference returns after printing "No valid points
    for alignment" (status 1) or "Error fitting RANSACRegressor" (status 2); nothing is printed here.  ``subsets`` / ``seed``: see
    ``ransac_scale_batch``."""
    dev = relative_depth.device if isinstance(relative_depth, torch.Tensor) and relative_depth.is_cuda else _dev(None)
    rel = _as_dev(relative_depth, torch.float32, dev)
    met = _as_dev(metric_depth, torch.float32, dev)
    if rel.dim() < 2 or rel.shape != met.shape:
        raise ValueError("relative_depth and metric_depth must be stacks of equal shape (P, ...)")
    m = None if mask is None else _as_dev(mask, torch.uint8, dev)
    if m is not None and m.shape != rel.shape:
        raise ValueError("mask must have the shape of the depth stack")
    P = rel.shape[0]
    n = rel[0].numel() if P else 0
    ro, mo, cnt = align_select_batch(rel, met, m, max_valid_depth, device=dev, stream=stream)
    res = ransac_scale_batch(ro, mo, cnt, min_samples, max_trials, subsets, seed, stream)
    out = torch.empty_like(rel)
    with torch.cuda.device(dev):
        check(lib.la3d_align_apply_batch(_ptr(rel), _ptr(met), _ptr(m), P, n, _ptr(res.coef), _ptr(res.status), 10000.0, _ptr(out),
                                         _stream(stream)), "la3d_align_apply_batch")
    _record(stream, rel, met, m, out)
    return out, res


class PlaneFit(NamedTuple):
    """Result of ``plane_ransac_batch`` / ``ground_planes``, device tensors with one row per image: ``plane`` float64 (P,4) =
    (n_x, n_y, n_z, d) with n . x + d = 0, |n| = 1 and n_y <= 0 (four NaN where status != 0); ``k_trial`` (inliers of the best trial),
    ``n_inliers`` (inliers of the reported plane), ``best_trial`` (-1 where status != 0) and ``status`` int32 - 0 fitted, 1 fewer than
    three samples, 2 no accepted trial or too few inliers, 3 a broken row -; ``rms`` float64 (NaN where status != 0); ``inliers`` uint8
    (P,n) flags of the reported plane's inliers, or None when they were not asked for."""
    plane: torch.Tensor
    k_trial: torch.Tensor
    n_inliers: torch.Tensor
    best_trial: torch.Tensor
    rms: torch.Tensor
    status: torch.Tensor
    inliers: Optional[torch.Tensor]

    def for_instances(self, image_index) -> torch.Tensor:
        """The (B,4) float64 device tensor the fit entries take as ``ground``: row b is the plane of image ``image_index[b]`` (a
        device ``index_select``, no host read-back).  Rows of images that were not fitted stay NaN, which the fit reads as "no ground"."""
        ii = _as_dev(image_index, torch.int64, self.plane.device).reshape(-1)
        return self.plane.index_select(0, ii)


def plane_select_batch(depth, K, candidates=None, step: int = 4, near: float = 0.0, far: float = float("inf"), stream=None):
    """The samples of the plane fit (C-ABI ``la3d_plane_select_batch``): ``depth`` (P,H,W) float32, ``K`` (3,3) or (P,3,3) ->
    ``(points (P,cap,3) float64, pixel (P,cap) int32, counts (P,) int64)`` on the GPU, cap = ceil(H/step) * ceil(W/step).  Image p's
    samples are the grid pixels (v % step == 0, u % step == 0) in raster order with a finite depth > 0 inside [near, far] and - with
    ``candidates``, a ``MaskBits`` of P planes whose stored width is a multiple of 32 (``frame_pad=True``) and whose ``frame_width`` is
    W, e.g. ``pack_label_bits(panoptic, ids=floor_and_road_ids)`` - a set candidate bit; ``points[p, :counts[p]]`` are the rows of
    ``unproject(depth, K)`` at ``pixel[p, :counts[p]]`` (= v * W + u), bit for bit.  Slots behind ``counts[p]`` are not written.  No
    host synchronisation."""
    dev = depth.device if isinstance(depth, torch.Tensor) and depth.is_cuda else _dev(None)
    d = _as_dev(depth, torch.float32, dev)
    if d.dim() != 3:
        raise ValueError("depth must be a (P,H,W) stack")
    P, H, W = d.shape
    k = _as_dev(K, torch.float64, dev, cache=True).reshape(-1, 9)
    if k.shape[0] not in (1, P):
        raise ValueError("K must be (3,3) or (P,3,3)")
    cb, cw, cs = None, 0, 0
    if candidates is not None:
        if not (isinstance(candidates, tuple) and len(candidates) == 4):
            raise ValueError("candidates must be a MaskBits (bits, H, W, frame_width)")
        mb = MaskBits(candidates[0], int(candidates[1]), int(candidates[2]), int(candidates[3]))
        cb = _as_dev(mb.bits, torch.int32, dev)
        if cb.dim() != 2 or cb.shape[0] != P or mb.H != H or mb.frame_width != W or mb.W % 32 != 0 or cb.shape[1] < H * mb.W // 32:
            raise ValueError("candidates must hold one plane per image of the depth's size, stored with a width that is a multiple of 32")
        cw, cs = mb.W, int(cb.shape[1])
    step = int(step)
    cap = (-(-H // step)) * (-(-W // step)) if step >= 1 else 0
    pts = torch.empty((P, cap, 3), dtype=torch.float64, device=dev)
    pix = torch.empty((P, cap), dtype=torch.int32, device=dev)
    cnt = torch.empty(P, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.la3d_plane_select_workspace_bytes(P, H, W, step)), dtype=torch.uint8, device=dev)
    a = PlaneSelectArgs(struct_size=C.sizeof(PlaneSelectArgs), P=P, H=H, W=W, step=step, k_stride=9 if k.shape[0] > 1 else 0,
                        near_depth=float(near), far_depth=float(far), depth=d.data_ptr(), K=k.data_ptr(),
                        candidates=None if cb is None else cb.data_ptr(), cand_plane_stride=cs, cand_width=cw,
                        points=pts.data_ptr(), pixel=pix.data_ptr(), counts=cnt.data_ptr(), workspace=ws.data_ptr())
    with torch.cuda.device(dev):
        a.stream = _stream(stream).value
        check(lib.la3d_plane_select_batch(C.byref(a)), "la3d_plane_select_batch")
    _record(stream, d, k, cb, pts, pix, cnt, ws)
    return pts, pix, cnt


def plane_ransac_batch(points, counts, threshold: float = 0.02, threshold_rel: float = 0.0, max_trials: int = 256, max_tilt=None,
                       min_inliers: int = 3, subsets=None, seed: int = 0, inliers: bool = False, stream=None) -> PlaneFit:
    """Batched RANSAC plane fit on the GPU (C-ABI ``la3d_plane_ransac_batch``; semantics in include/la3d.h): ``points`` (P,n,3) float64
    and ``counts`` (P,) int64 as ``plane_select_batch`` leaves them, or from any other source.  A sample at depth z is an inlier within
    ``threshold + threshold_rel * z`` of the plane; ``max_tilt`` (radians, None = any) is the largest angle between the plane's normal and
    the camera's y axis - the prior that keeps walls out; ``min_inliers`` the fewest inliers of the best trial that count as a fit.
    ``subsets``: int32 (P, max_trials, 3) sample indices per trial, or None: drawn on the device from ``seed`` -
    ``ransac_subsets(counts, 3, max_trials, seed)`` exports exactly that draw.  All trials are judged; the best plane is refitted over
    its inliers (covariance about their mean, smallest eigenvector) and oriented so that n_y <= 0.  ``inliers=True`` also returns the
    flags.  No host synchronisation; returns a ``PlaneFit`` of device tensors."""
    dev = points.device if isinstance(points, torch.Tensor) and points.is_cuda else _dev(None)
    x = _as_dev(points, torch.float64, dev)
    if x.dim() != 3 or x.shape[2] != 3:
        raise ValueError("points must be (P, n, 3)")
    P, n = int(x.shape[0]), int(x.shape[1])
    cnt = _as_dev(counts, torch.int64, dev).reshape(-1)
    if cnt.numel() != P:
        raise ValueError("counts must hold one entry per point set")
    sub = None
    if subsets is not None:
        sub = _as_dev(subsets, torch.int32, dev)
        if sub.shape != (P, int(max_trials), 3):
            raise ValueError("subsets must be (P, max_trials, 3)")
    cos2 = 0.0 if max_tilt is None else float(np.cos(np.float64(max_tilt)) ** 2)
    plane = torch.empty((P, 4), dtype=torch.float64, device=dev)
    rms = torch.empty(P, dtype=torch.float64, device=dev)
    ints = torch.empty((4, P), dtype=torch.int32, device=dev)
    flags = torch.empty((P, n), dtype=torch.uint8, device=dev) if inliers else None
    ws = torch.empty(int(lib.la3d_plane_ransac_workspace_bytes(P, n, int(max_trials))), dtype=torch.uint8, device=dev)
    a = PlaneRansacArgs(struct_size=C.sizeof(PlaneRansacArgs), P=P, n=n, points=x.data_ptr(), counts=cnt.data_ptr(),
                        thr_abs=float(threshold), thr_rel=float(threshold_rel), cos2_tilt=cos2, max_trials=int(max_trials),
                        min_inliers=int(min_inliers), subsets=None if sub is None else sub.data_ptr(), seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                        plane=plane.data_ptr(), k_trial=ints[0].data_ptr(), n_inliers=ints[1].data_ptr(), best_trial=ints[2].data_ptr(),
                        rms=rms.data_ptr(), status=ints[3].data_ptr(), inliers=None if flags is None else flags.data_ptr(),
                        workspace=ws.data_ptr())
    with torch.cuda.device(dev):
        a.stream = _stream(stream).value
        check(lib.la3d_plane_ransac_batch(C.byref(a)), "la3d_plane_ransac_batch")
    _record(stream, x, cnt, sub, plane, rms, ints, flags, ws)
    return PlaneFit(plane, ints[0], ints[1], ints[2], rms, ints[3], flags)


def ground_planes(depth, K, candidates=None, step: int = 4, near: float = 0.0, far: float = float("inf"), threshold: float = 0.02,
                  threshold_rel: float = 0.0, max_trials: int = 256, max_tilt=None, min_inliers: int = 3, seed: int = 0,
                  inliers: bool = False, stream=None) -> PlaneFit:
    """The dominant plane of every image of a (P,H,W) float32 depth stack - the floor or the road of most scenes -, every step on the
    GPU and without any host read-back: ``plane_select_batch`` -> ``plane_ransac_batch`` (their arguments).  ``candidates``: a
    ``MaskBits`` of the pixels that may be ground (the floor / road ids of a panoptic label map through ``pack_label_bits``).
    ``gp.for_instances(image_index)`` is the ``ground`` argument of the fit entries; ``inliers`` flags index the samples of the select,
    not the pixels."""
    pts, _, cnt = plane_select_batch(depth, K, candidates, step, near, far, stream)
    return plane_ransac_batch(pts, cnt, threshold, threshold_rel, max_trials, max_tilt, min_inliers, None, seed, inliers, stream)


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


def _as_batch(x):
    return x[None] if isinstance(x, torch.Tensor) else np.asarray(x)[None]


def depth_match_transform(mask, depth_map, R, T, render_alpha_mask, depth_render):
    """``align_to_depth_match`` (reference src/util.py:464-494) after its ``process_object`` call: returns the 4x4 transform
    ``[inv(R[:3,:3]) * scale | T[:3] * scale]`` with ``scale`` the median depth ratio over ``mask & render_alpha_mask``, or
    ``np.eye(4)`` (and the reference's message) when the two masks do not overlap."""
    med, cnt = masked_ratio_median(_as_batch(depth_map), _as_batch(depth_render), _as_batch(mask), _as_batch(render_alpha_mask))
    if int(cnt[0]) == 0:
        print("No overlap between masks found")
        return np.eye(4)
    scale = np.float32(med[0].item())   # a float32 value, as np.median of a float32 array
    transform = np.eye(4)
    transform[:3, :3] = np.linalg.inv(np.asarray(R)[:3, :3]) * scale
    transform[:3, -1] = np.asarray(T)[:3] * scale
    return transform
