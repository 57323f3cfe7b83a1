"""CPU-only: the NumPy restatement of the batched RANSAC scale fit (tests/align_ransac_cases.py - the semantics the device code
follows) against scikit-learn's ``RANSACRegressor(LinearRegression(fit_intercept=False))`` itself, fed the same seeded generator.

Family: n in FAMILY_N x min_samples in (0.05, 0.2, 0.5) x outlier share in (0, 0.3, 0.6) x 6 seeds = 648 cases.

Coefficient tolerance: both sides solve the same least-squares problem over the same inliers, scikit-learn with LAPACK's float32
``gelsd``, the restatement with float64 sums rounded once.  The worst relative difference this sweep measures over the family is
3.8e-7 (about 3 float32 ulp; 4.3e-7 on the 599-case family the feature was planned on); the tolerance is four times the measured
value: COEF_RTOL = 1.52e-6.  In the sweep scikit-learn raised in 0 of the 648 cases and 0 picked another trial than scikit-learn; a
case in which scikit-learn raises has a test of its own below.
"""
import warnings

import numpy as np
import pytest

from . import align_ransac_cases as R

COEF_RTOL = R.COEF_RTOL
SEEDS = range(6)


def _sklearn_fit(x, y, min_samples, seed):
    from sklearn.linear_model import LinearRegression, RANSACRegressor

    reg = RANSACRegressor(estimator=LinearRegression(fit_intercept=False), min_samples=min_samples,
                          random_state=np.random.RandomState(seed))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        reg.fit(x.reshape(-1, 1), y.reshape(-1, 1))
    return reg


def _compare(n, min_samples, outliers, seed):
    """(raised, trial_differs, relative coefficient difference) of one case; asserts the rest."""
    x, y = R.make_case(n, outliers, 1000 * n + seed)
    m = R.subset_size(min_samples, n)
    subsets = R.host_subsets(np.random.RandomState(seed), n, m, 100) if 1 <= m <= n else np.zeros((100, 1), np.int32)
    got = R.ransac_scale(x, y, subsets, min_samples)
    try:
        reg = _sklearn_fit(x, y, min_samples, seed)
    except ValueError:
        assert got["status"] == R.FAILED, (n, min_samples, outliers, seed)
        return True, False, 0.0
    assert got["status"] == R.OK, (n, min_samples, outliers, seed)
    k_ref = int(reg.inlier_mask_.sum())
    if got["n_trials"] != reg.n_trials_ or got["n_inliers"] != k_ref:
        return False, True, 0.0            # another trial chosen: a float32-versus-float64 score tie, counted against the cap
    c_ref = float(np.asarray(reg.estimator_.coef_).reshape(-1)[0])
    return False, False, abs(float(got["coef"]) - c_ref) / abs(c_ref)


_seen = {"cases": 0, "differ": 0, "worst": 0.0}


@pytest.mark.parametrize("n", R.FAMILY_N)
def test_restatement_equals_sklearn(n):
    for ms in R.FAMILY_MIN_SAMPLES:
        for out in R.FAMILY_OUTLIERS:
            for seed in SEEDS:
                raised, differs, rel = _compare(n, ms, out, seed)
                _seen["cases"] += 1
                _seen["differ"] += int(differs)
                _seen["worst"] = max(_seen["worst"], rel)
                assert rel <= COEF_RTOL, (n, ms, out, seed, rel)
    # at most 1 % of the family may pick another trial than scikit-learn (score ties between float32 and float64 sums)
    assert _seen["differ"] * 100 <= max(_seen["cases"], 648), _seen


def test_early_stop_shows_at_small_n():
    x, y = R.make_case(40, 0.0, 7)
    got = R.ransac_scale(x, y, R.host_subsets(np.random.RandomState(3), 40, 8, 100), 0.2)
    assert got["status"] == R.OK and got["n_trials"] < 100


def test_failed_and_empty_fits():
    x, y = R.make_case(12, 0.3, 1)
    sub = R.host_subsets(np.random.RandomState(0), 12, 3, 100)
    assert R.ransac_scale(x[:0], y[:0], sub, 0.2)["status"] == R.EMPTY
    assert R.ransac_scale(x, y, sub, 13)["status"] == R.FAILED            # m > n
    xn = x.copy()
    xn[4] = np.nan
    assert R.ransac_scale(xn, y, sub, 0.2)["status"] == R.FAILED          # scikit-learn raises on a non-finite sample
    yn = y.copy()
    yn[2] = -np.inf
    assert R.ransac_scale(x, yn, sub, 0.2)["status"] == R.FAILED
    bad = sub.copy()
    bad[5, 1] = 12
    assert R.ransac_scale(x, y, bad, 0.2)["status"] == R.FAILED           # an index outside [0, n)
    assert R.ransac_scale(x, y, sub, 3)["status"] == R.OK                 # an integer min_samples


def test_sklearn_raises_where_the_restatement_fails():
    """No consensus set: more than half of the y are equal, so the threshold is 0 and no trial has an inlier - scikit-learn raises
    (the reference catches it and returns the metric depth), the restatement reports status 2 after looking at all 100 trials."""
    rs = np.random.RandomState(4)
    x = rs.uniform(0.5, 4.0, 31).astype(np.float32)
    y = np.full(31, 2.0, np.float32)
    y[:9] = rs.uniform(0.1, 30.0, 9).astype(np.float32)
    with pytest.raises(ValueError):
        _sklearn_fit(x, y, 0.2, 0)
    got = R.ransac_scale(x, y, R.host_subsets(np.random.RandomState(0), 31, 7, 100), 0.2)
    assert got["status"] == R.FAILED and got["n_trials"] == 100 and got["best_trial"] == -1


def test_dynamic_max_trials_is_sklearns():
    from sklearn.linear_model._ransac import _dynamic_max_trials

    for k, n, m in ((1, 40, 8), (30, 40, 8), (40, 40, 8), (200000, 307200, 61440), (5, 5, 1), (3, 7, 2)):
        assert R.dynamic_max_trials(k, n, m) == _dynamic_max_trials(k, n, m, 0.99)


# ---- the hostile families of the differential campaign (oracle/campaigns/align_ransac.py) at n <= 1025 -----------------------------------
HOSTILE_N = (1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
HOSTILE_MIN_SAMPLES = (0.05, 0.2, 0.5, 1, 2)
_hostile = {"cases": 0, "differ": 0, "worst": 0.0, "raised": 0, "thr0": 0, "thr0 agree": 0, "thr0 sklearn raises, restatement fits": 0,
            "thr0 other coefficient": 0, "f32 overflow": 0, "f32 overflow agree": 0}
F32_MAX = float(np.finfo(np.float32).max)


def _compare_hostile(family, n, min_samples):
    rs = np.random.RandomState(HOSTILE_N.index(n) * 16 + HOSTILE_MIN_SAMPLES.index(min_samples))
    x, y = R.FAMILIES[family](rs, n)
    m = R.subset_size(min_samples, n)
    seed = n + 7
    subsets = R.host_subsets(np.random.RandomState(seed), n, m, 100) if 1 <= m <= n else np.zeros((100, 1), np.int32)
    trace = []
    got = R.ransac_scale(x, y, subsets, min_samples, trace=trace)                     # (never raises)
    assert got["status"] in (R.OK, R.FAILED) and (got["status"] != R.OK or np.isfinite(got["coef"])), (family, n, min_samples, got)
    try:
        reg = _sklearn_fit(x, y, min_samples, seed)
        c_ref, k_ref, t_ref = float(np.asarray(reg.estimator_.coef_).reshape(-1)[0]), int(reg.inlier_mask_.sum()), reg.n_trials_
    except ValueError:
        reg = None
    if 1 <= m <= n and float(R.threshold(y)) == 0.0:
        # the zero-threshold class: the inlier test is an exact float32 equality and hangs on the last bit of the slope, where LAPACK's
        # float32 gelsd and float32(sum xy / sum xx) differ - counted, not asserted
        _hostile["thr0"] += 1
        if reg is None:
            _hostile["thr0 agree" if got["status"] == R.FAILED else "thr0 sklearn raises, restatement fits"] += 1
        else:
            same = got["status"] == R.OK and got["n_inliers"] == k_ref and abs(float(got["coef"]) - c_ref) <= COEF_RTOL * abs(c_ref)
            _hostile["thr0 agree" if same else "thr0 other coefficient"] += 1
        return
    same_set = reg is not None and got["status"] == R.OK and np.array_equal(
        next(ev["inl"] for ev in trace if ev["t"] == got["best_trial"]), np.asarray(reg.inlier_mask_).reshape(-1))
    if 1 <= m <= n and float((y.astype(np.float64) ** 2).sum()) >= F32_MAX:
        # outside float32's range: scikit-learn scores float32 targets in float32, sum y^2 overflows, its scores are inf or NaN and its
        # choice among trials of equal k is no longer by R^2; the library scores in float64 - counted, not asserted
        _hostile["f32 overflow"] += 1
        _hostile["f32 overflow agree"] += int(same_set and abs(float(got["coef"]) - c_ref) <= COEF_RTOL * abs(c_ref))
        return
    _hostile["cases"] += 1
    if reg is None:
        assert got["status"] == R.FAILED, (family, n, min_samples, got)
        _hostile["raised"] += 1
        return
    assert got["status"] == R.OK, (family, n, min_samples, got)
    if got["n_trials"] != t_ref or got["n_inliers"] != k_ref or not same_set:
        _hostile["differ"] += 1                                                         # counted against the 1 % cap
        return
    rel = abs(float(got["coef"]) - c_ref) / abs(c_ref) if c_ref != 0.0 else abs(float(got["coef"]))
    _hostile["worst"] = max(_hostile["worst"], rel)
    assert rel <= COEF_RTOL, (family, n, min_samples, rel)


@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_restatement_equals_sklearn_on_the_hostile_families(family):
    """Every family of the campaign x 16 sizes x 5 min_samples = 960 cases against scikit-learn on the same seeded subsets.  With a
    threshold above zero scikit-learn raises exactly where the restatement reports status 2, at most 1 % of the cases pick another
    trial or inlier set (measured: 1 of 686), and the coefficient lies within the unchanged COEF_RTOL (worst measured 7.5e-7
    relative, on x 1e15 / y 1e16).  With a zero threshold (one sample, constant y, more than half of the y equal: 199 cases, 14 disagreements) and where
    sum y^2 leaves float32's range (75 cases, 6 disagreements) the two may part - see the module docstring of
    tests/align_ransac_cases.py -: agreements and disagreements are counted and printed, and the restatement must neither raise nor
    report a non-finite coefficient with status 0."""
    for n in HOSTILE_N:
        for ms in HOSTILE_MIN_SAMPLES:
            _compare_hostile(family, n, ms)
    print(_hostile)
    assert _hostile["differ"] * 100 <= max(_hostile["cases"], 600), _hostile
