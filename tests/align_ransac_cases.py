"""The batched RANSAC scale fit (include/la3d.h "depth alignment: RANSAC scale fit") restated with NumPy: the one text that the device
code (labelany3d_amd/csrc/la3d_align.hip) and the tests follow.  It is scikit-learn's ``RANSACRegressor(LinearRegression(
fit_intercept=False), min_samples=...)`` on float32 samples, fed its subsets explicitly; tests/test_align_ransac_restatement.py
compares it with scikit-learn itself.

Status: 0 fitted, 1 no valid sample, 2 the fit failed (what the reference's ``align_depth`` catches and answers with the metric depth).
"""
import math

import numpy as np

OK, EMPTY, FAILED = 0, 1, 2
# relative coefficient tolerance against scikit-learn (LAPACK's float32 gelsd against float64 sums rounded once): four times the
# worst case the sweep of tests/test_align_ransac_restatement.py measures (3.8e-7)
COEF_RTOL = 4 * 3.8e-7
_EPS = float(np.spacing(1))


def subset_size(min_samples, n):
    """m of a frame with n samples: ceil(min_samples * n) in float64 for 0 < min_samples < 1, min_samples itself from 1 on."""
    if 0 < min_samples < 1:
        return int(np.ceil(np.float64(min_samples) * np.float64(n)))
    return int(min_samples)


def dynamic_max_trials(k, n, m, probability=0.99):
    """scikit-learn's ``_dynamic_max_trials`` in float64."""
    ratio = k / float(n)
    nom = max(_EPS, 1 - probability)
    denom = max(_EPS, 1 - ratio ** m)
    if nom == 1:
        return 0
    if denom == 1:
        return float("inf")
    return abs(float(np.ceil(np.log(nom) / np.log(denom))))


def slope(x, y):
    """float32(sum x*y / sum x*x), sums in float64; 0 where sum x*x is 0 (the minimum-norm solution)."""
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    sxx = float((xd * xd).sum())
    if sxx == 0.0:
        return np.float32(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(float((xd * yd).sum()) / sxx)


def score_r2(y_in, pred_in):
    """R^2 over the inliers in float64 with scikit-learn's special values."""
    k = y_in.size
    if k < 2:
        return float("nan")
    yd, pd = y_in.astype(np.float64), pred_in.astype(np.float64)
    num = float(((yd - pd) ** 2).sum())
    den = float(((yd - yd.mean()) ** 2).sum())
    if den == 0.0:
        return 1.0 if num == 0.0 else 0.0
    return 1.0 - num / den


def threshold(y):
    """median(|y - median(y)|) of float32 data in float32."""
    y = np.asarray(y, np.float32)
    return np.median(np.abs(y - np.median(y)))


def ransac_scale(x, y, subsets, min_samples=0.2, max_trials=100, stop_probability=0.99):
    """One frame.  x, y: float32 (n,), subsets: int (T, >= m) - trial t uses subsets[t, :m].
    Returns dict(status, coef, n_inliers, n_trials, best_trial)."""
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
    k_best, score_best, best, a_best = 1, -math.inf, -1, None
    limit, t = max_trials, 0
    while t < limit:
        idx = subsets[t, :m]
        t += 1
        a = slope(x[idx], y[idx])
        pred = x * a                                  # one rounded float32 product per sample
        with np.errstate(invalid="ignore", over="ignore"):
            inl = np.abs(y - pred) <= thr
        k = int(inl.sum())
        if k < k_best:
            continue
        s = score_r2(y[inl], pred[inl])
        if k == k_best and s < score_best:
            continue
        k_best, score_best, best, a_best = k, s, t - 1, a
        limit = min(limit, dynamic_max_trials(k_best, n, m, stop_probability))
    if best < 0:
        return dict(fail, n_trials=t)
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
