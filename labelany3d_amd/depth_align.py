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
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from ._device import _as_dev, _dev, _ptr, _record, _stream
from ._lib import AlignRansacArgs, check, lib


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
