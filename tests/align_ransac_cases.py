"""The batched RANSAC scale fit (include/la3d.h "depth alignment: RANSAC scale fit") restated with NumPy: the one text that the device
code (labelany3d_amd/csrc/la3d_align.hip) and the tests follow.  It is scikit-learn's ``RANSACRegressor(LinearRegression(
fit_intercept=False), min_samples=...)`` on float32 samples, fed its subsets explicitly; tests/test_align_ransac_restatement.py
compares it with scikit-learn itself.

Status: 0 fitted, 1 no valid sample, 2 the fit failed (what the reference's ``align_depth`` catches and answers with the metric depth).

Where the restatement (and with it the library) parts from scikit-learn - tests/test_align_ransac_restatement.py counts both classes:
* thr == 0 (one sample, constant y, more than half of the y equal): the inlier test ``|y - pred| <= 0`` is the exact float32 equality
  ``y == float32(x * a)`` and hangs on the last bit of the slope, where ``float32(sum xy / sum xx)`` and LAPACK's float32 ``gelsd``
  differ.  scikit-learn may raise "no consensus set" (the reference then returns the metric depth) where this text reports status 0
  with as few as one inlier, or both fit with different coefficients (up to 1.7 x apart on constant y).
* sum y^2 outside float32's range (|y| of the order 1e19): scikit-learn scores float32 targets in float32, its scores are inf or NaN
  and its choice among trials of equal k is arbitrary; the scores here are float64.
The device code is held to THIS text in both classes (oracle/campaigns/align_ransac.py).
"""
import math

import numpy as np

OK, EMPTY, FAILED = 0, 1, 2
# relative coefficient tolerance against scikit-learn (LAPACK's float32 gelsd against float64 sums rounded once): four times the
# worst case the sweep of tests/test_align_ransac_restatement.py measures (3.8e-7; the hostile families of the campaign reach 7.5e-7)
COEF_RTOL = 4 * 3.8e-7
_EPS = float(np.spacing(1))


def subset_size(min_samples, n):
    """m of a frame with n samples: ceil(min_samples * n) in float64 for 0 < min_samples < 1, min_samples itself from 1 on."""
    if 0 < min_samples < 1:
        return int(np.ceil(np.float64(min_samples) * np.float64(n)))
    return int(min_samples)


def limit_quotient(k, n, m, probability=0.99):
    """``log(nom) / log(denom)`` of scikit-learn's ``_dynamic_max_trials`` in float64 - the number its ``ceil`` rounds -, or the special
    value it returns instead: 0 for a stop probability of 0, inf where ``(k / n) ** m`` underflows."""
    ratio = k / float(n)
    nom = max(_EPS, 1 - probability)
    denom = max(_EPS, 1 - ratio ** m)
    if nom == 1:
        return 0
    if denom == 1:
        return float("inf")
    return float(np.log(nom) / np.log(denom))


def dynamic_max_trials(k, n, m, probability=0.99):
    """scikit-learn's ``_dynamic_max_trials`` in float64."""
    q = limit_quotient(k, n, m, probability)
    return q if q == 0 or q == float("inf") else abs(float(np.ceil(q)))


def slope_quotient(x, y):
    """sum x*y / sum x*x in float64 - the number ``slope`` rounds to float32 -, None where sum x*x is 0."""
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    sxx = float((xd * xd).sum())
    if sxx == 0.0:
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        return float((xd * yd).sum()) / sxx


def slope(x, y):
    """float32(sum x*y / sum x*x), sums in float64; 0 where sum x*x is 0 (the minimum-norm solution)."""
    q = slope_quotient(x, y)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(0.0) if q is None else np.float32(q)


def score_r2(y_in, pred_in, parts=None):
    """R^2 over the inliers in float64 with scikit-learn's special values.  ``parts``: a dict that receives the two sums."""
    k = y_in.size
    if k < 2:
        return float("nan")
    yd, pd = y_in.astype(np.float64), pred_in.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        num = float(((yd - pd) ** 2).sum())
        den = float(((yd - yd.mean()) ** 2).sum())
    if parts is not None:
        parts.update(num=num, den=den)
    if den == 0.0:
        return 1.0 if num == 0.0 else 0.0
    return 1.0 - num / den


def threshold(y):
    """median(|y - median(y)|) of float32 data in float32."""
    y = np.asarray(y, np.float32)
    return np.median(np.abs(y - np.median(y)))


def ransac_scale(x, y, subsets, min_samples=0.2, max_trials=100, stop_probability=0.99, trace=None, alt=None):
    """One frame.  x, y: float32 (n,), subsets: int (T, >= m) - trial t uses subsets[t, :m].
    Returns dict(status, coef, n_inliers, n_trials, best_trial).

    ``trace``: a list that receives one dict per trial the loop looked at (its slope and the float64 quotient behind it, k, the score
    with its two sums, the best it was compared with, the quotient of the trial limit it set) - what oracle/campaigns/align_ransac.py
    classifies a frame by.  ``alt``: dict(flip={t}, slope={t: a}, limit={t: L}) walks the same loop with the score comparison of the
    trials in ``flip`` answered the other way, the slope of a trial replaced (the neighbouring float32) or the limit a trial sets
    replaced (the neighbouring integer): the outcomes a frame may have where one of them hangs on float64 rounding."""
    x, y = np.asarray(x, np.float32).reshape(-1), np.asarray(y, np.float32).reshape(-1)
    n = x.size
    fail = dict(status=FAILED, coef=np.float32("nan"), n_inliers=0, n_trials=0, best_trial=-1)
    if n == 0:
        return dict(fail, status=EMPTY)
    m = subset_size(min_samples, n)
    if m < 1 or m > n or not (np.isfinite(x).all() and np.isfinite(y).all()):
        return fail
    subsets = np.asarray(subsets)
    if subsets.shape[1] < m or (subsets[:max_trials, :m] < 0).any() or (subsets[:max_trials, :m] >= n).any():
        return fail
    thr = threshold(y)
    alt = alt or {}
    k_best, score_best, best, a_best = 1, -math.inf, -1, None
    limit, t = max_trials, 0
    while t < limit:
        idx = subsets[t, :m]
        t += 1
        a = alt.get("slope", {}).get(t - 1, slope(x[idx], y[idx]))
        with np.errstate(invalid="ignore", over="ignore"):
            pred = x * a                              # one rounded float32 product per sample
            inl = np.abs(y - pred) <= thr
        k = int(inl.sum())
        ev = None
        if trace is not None:
            ev = dict(t=t - 1, a=a, q=slope_quotient(x[idx], y[idx]), k=k, s=None, parts={}, k_best=k_best, score_best=score_best,
                      best=best, a_best=a_best, accepted=False, limit_q=None, inl=inl)
            trace.append(ev)
        if k < k_best:
            continue
        s = score_r2(y[inl], pred[inl], None if ev is None else ev["parts"])
        if ev is not None:
            ev["s"] = s
        worse = k == k_best and s < score_best
        if (t - 1) in alt.get("flip", ()):
            worse = k == k_best and not worse
        if worse:
            continue
        k_best, score_best, best, a_best = k, s, t - 1, a
        lim = alt.get("limit", {}).get(t - 1, dynamic_max_trials(k_best, n, m, stop_probability))
        limit = min(limit, lim)
        if ev is not None:
            ev.update(accepted=True, limit_q=limit_quotient(k_best, n, m, stop_probability),
                      limit_same=max(_EPS, 1 - stop_probability) == max(_EPS, 1 - (k_best / float(n)) ** m))
    if best < 0:
        return dict(fail, n_trials=t)
    with np.errstate(invalid="ignore", over="ignore"):
        pred = x * a_best
        inl = np.abs(y - pred) <= thr
    return dict(status=OK, coef=slope(x[inl], y[inl]), n_inliers=k_best, n_trials=t, best_trial=best)


def host_subsets(rng, n, m, trials):
    """The subsets scikit-learn's loop draws from ``rng`` (a RandomState, or the module ``np.random`` for the global stream): ``trials``
    calls of ``sample_without_replacement(n, m)``, as an int32 (trials, m) array."""
    from sklearn.utils import check_random_state
    from sklearn.utils.random import sample_without_replacement

    rs = check_random_state(rng)
    return np.stack([sample_without_replacement(n, m, random_state=rs) for _ in range(trials)]).astype(np.int32)


FAMILY_N = (3, 4, 5, 7, 12, 19, 40, 63, 64, 65, 130, 257)
FAMILY_MIN_SAMPLES = (0.05, 0.2, 0.5)
FAMILY_OUTLIERS = (0.0, 0.3, 0.6)


def make_case(n, outliers, seed, scale=2.5):
    """Seeded samples: y = scale * x + noise, a share of outliers drawn uniformly."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(0.5, 4.0, n).astype(np.float32)
    y = (scale * x + 0.05 * rs.randn(n)).astype(np.float32)
    o = rs.rand(n) < outliers
    y[o] = rs.uniform(0.1, 30.0, int(o.sum())).astype(np.float32)
    return x, y


# ---- the hostile families (shared by oracle/campaigns/align_ransac.py and tests/test_align_ransac_restatement.py) --------------------
def _line(rs, n, outliers, scale=2.5):
    x = rs.uniform(0.5, 4.0, n).astype(np.float32)
    y = (scale * x + 0.05 * rs.randn(n)).astype(np.float32)
    o = rs.rand(n) < outliers
    y[o] = rs.uniform(0.1, 30.0, int(o.sum())).astype(np.float32)
    return x, y


def _quantised(rs, n):
    """x in quarter, y in half steps: heavy ties in both medians and among the residuals."""
    x, y = _line(rs, n, 0.3)
    return (np.round(x * 4) / 4).astype(np.float32), (np.round(y * 2) / 2).astype(np.float32)


def _y_majority(rs, n):
    """More than half of the y equal: thr == 0.  Even draw of the coin: the rest lies anywhere (no trial has an inlier unless a product
    happens to be exact); odd: all samples on the exact line y = 2 x over dyadic x, so every subset's slope is 2 and every sample fits."""
    k = n // 2 + 1
    if rs.randint(2):
        x = (rs.randint(1, 64, n) / 8.0).astype(np.float32)
        x[rs.permutation(n)[:k]] = 1.5
        return x, (2.0 * x).astype(np.float32)
    x, y = _line(rs, n, 0.3)
    y[rs.permutation(n)[:k]] = 2.0
    return x, y


def _exact(rs, n):
    """y = 2.5 x exactly over dyadic x: thr > 0 (unless n < 3), every residual 0, every slope 2.5."""
    x = (rs.randint(1, 256, n) / 8.0).astype(np.float32)
    return x, (2.5 * x).astype(np.float32)


def _const_y(rs, n):
    return rs.uniform(0.5, 4.0, n).astype(np.float32), np.full(n, 3.0, np.float32)


def _x_half_zero(rs, n):
    x, y = _line(rs, n, 0.1)
    x[rs.rand(n) < 0.5] = 0.0
    return x, y


def _signed(rs, n):
    x, y = _line(rs, n, 0.1)
    return -x, (y * rs.choice([-1.0, 1.0], n)).astype(np.float32)


def _scaled(fx, fy):
    def f(rs, n):
        x, y = _line(rs, n, 0.3)
        return (x * np.float32(fx)).astype(np.float32), (y * np.float32(fy)).astype(np.float32)
    return f


# name -> f(rs, n) -> (x, y) float32 (n,)
FAMILIES = {
    "clean": lambda rs, n: _line(rs, n, 0.0),
    "outliers 30 %": lambda rs, n: _line(rs, n, 0.3),
    "outliers 60 %": lambda rs, n: _line(rs, n, 0.6),
    "quantised": _quantised,
    "y majority equal": _y_majority,
    "exact dyadic line": _exact,
    "constant y": _const_y,
    "half of x zero": _x_half_zero,
    "negative x, signed y": _signed,
    "x 1e15, y 1e16": _scaled(1e15, 1e16),     # the largest decade at which sum y^2 of 1025 samples stays inside float32 (scikit-learn's score)
    "x 1e18, y 1e19": _scaled(1e18, 1e19),
    "1e-20": _scaled(1e-20, 1e-20),
}
