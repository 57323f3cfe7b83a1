"""GPU tests of the batched RANSAC scale fit (include/la3d.h "depth alignment: RANSAC scale fit"; kernels:
labelany3d_amd/csrc/la3d_align.hip): ``ransac_scale_batch`` / ``ransac_subsets`` / ``align_depth_batch`` against the NumPy restatement
of the semantics (tests/align_ransac_cases.py, itself pinned against scikit-learn by tests/test_align_ransac_restatement.py), against
scikit-learn directly and against the reference-run fixture g10_align.npz."""
import ctypes as C
import warnings

import numpy as np
import pytest

from labelany3d_amd import RansacScale, align_depth_batch, ransac_scale_batch, ransac_subsets

from . import align_ransac_cases as R

pytestmark = pytest.mark.gpu

T = 100
SIZES = (3, 5, 12, 40, 63, 64, 65, 257, 4097)


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _host(res):
    return {k: getattr(res, k).cpu().numpy() for k in RansacScale._fields}


def _stack(cases, min_samples, rng_seed):
    """cases: list of (x, y) -> padded (P, n) sample rows, counts, explicit subsets (P, T, m_cap) drawn as scikit-learn draws them."""
    P, cap = len(cases), max(len(x) for x, _ in cases)
    xs, ys = np.zeros((P, cap), np.float32), np.zeros((P, cap), np.float32)
    counts = np.array([len(x) for x, _ in cases], np.int64)
    ms = [R.subset_size(min_samples, int(c)) for c in counts]
    sub = np.full((P, T, max(max(ms), 1)), -1, np.int32)
    for p_, (x, y) in enumerate(cases):
        xs[p_, :len(x)], ys[p_, :len(x)] = x, y
        if 1 <= ms[p_] <= len(x):
            sub[p_, :, :ms[p_]] = R.host_subsets(np.random.RandomState(rng_seed + p_), len(x), ms[p_], T)
    return xs, ys, counts, sub


def _ulp_apart(a, b):
    a, b = np.float32(a), np.float32(b)
    return a == b or np.nextafter(a, b) == b


@pytest.mark.parametrize("min_samples", [0.05, 0.2, 0.5, 3])
def test_explicit_subsets_equal_the_restatement(torch_gpu, min_samples):
    """Every size at which the kernels take another path (one lane, one wave, 63 / 64 / 65, one segment + 1 sample), in ONE batched
    call per min_samples: n_trials, n_inliers, best_trial and status equal the restatement's; coef equal or adjacent float32 (both
    sides round float64 quotients that differ by summation order only)."""
    cases = [R.make_case(n, 0.3, 100 + n) for n in SIZES]
    xs, ys, counts, sub = _stack(cases, min_samples, 7)
    got = _host(ransac_scale_batch(xs, ys, counts, min_samples, T, subsets=sub))
    for p_, (x, y) in enumerate(cases):
        want = R.ransac_scale(x, y, sub[p_], min_samples, T)
        for k in ("status", "n_trials", "n_inliers", "best_trial"):
            assert got[k][p_] == want[k], (len(x), k, got[k][p_], want[k])
        assert want["status"] == R.OK and _ulp_apart(got["coef"][p_], want["coef"]), (len(x), got["coef"][p_], want["coef"])
        if len(x) == 40 and min_samples == 0.05:
            assert want["n_trials"] < T          # the data-dependent early stop shows here


@pytest.mark.parametrize("trials", [1, 7, 64, 65, 1024])
def test_other_trial_counts(torch_gpu, trials):
    """max_trials other than 100: one trial, a ragged chunk of the 64-trial rows, one chunk and one more, and the entry's limit (the
    candidates pass then takes 148 KiB of LDS per workgroup)."""
    frames = [R.make_case(n, 0.3, 700 + n) for n in (257, 4097)]
    for x, y in frames:
        n = len(x)
        sub = R.host_subsets(np.random.RandomState(trials), n, R.subset_size(0.2, n), trials)
        got = _host(ransac_scale_batch(x[None], y[None], np.array([n]), 0.2, trials, subsets=sub[None]))
        want = R.ransac_scale(x, y, sub, 0.2, trials)
        for k in ("status", "n_trials", "n_inliers", "best_trial"):
            assert got[k][0] == want[k], (n, k, got[k][0], want[k])
        assert _ulp_apart(got["coef"][0], want["coef"])


def _sklearn(x, y, min_samples, seed):
    from sklearn.linear_model import LinearRegression, RANSACRegressor

    reg = RANSACRegressor(estimator=LinearRegression(fit_intercept=False), min_samples=min_samples, random_state=np.random.RandomState(seed))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        reg.fit(x.reshape(-1, 1), y.reshape(-1, 1))
    return reg


@pytest.mark.parametrize("n", [48 * 64, 4097])
def test_against_sklearn_directly(torch_gpu, n):
    x, y = R.make_case(n, 0.3, n)
    reg = _sklearn(x, y, 0.2, 21)
    sub = R.host_subsets(np.random.RandomState(21), n, R.subset_size(0.2, n), T)
    got = _host(ransac_scale_batch(x[None], y[None], np.array([n]), 0.2, T, subsets=sub[None]))
    assert got["status"][0] == 0 and got["n_trials"][0] == reg.n_trials_ and got["n_inliers"][0] == int(reg.inlier_mask_.sum())
    c_ref = float(np.asarray(reg.estimator_.coef_).reshape(-1)[0])
    assert abs(float(got["coef"][0]) - c_ref) <= R.COEF_RTOL * abs(c_ref)


def _valid(rel, met, mask, cap):
    v = (~np.isinf(rel)) & (met < cap)
    return v if mask is None else v & mask


@pytest.mark.parametrize("name", ["nomask", "mask", "lowcap", "novalid", "neginf"])
def test_align_depth_batch_vs_reference_run(torch_gpu, golden, name):
    """The frames of the reference run (tests/golden/make_golden_align.py) with the subsets its RANSAC drew from the seeded global NumPy
    stream: the aligned map equals the reference's within the coefficient tolerance of the CPU test."""
    g = golden("g10_align.npz")
    rel, met, mask = g[f"ad_{name}_rel"], g[f"ad_{name}_met"], g[f"ad_{name}_mask"]
    ms, cap, seed = g[f"ad_{name}_par"]
    mask = None if mask.size == 0 else mask
    n = int(_valid(rel, met, mask, cap).sum())
    sub = None
    if n:
        np.random.seed(int(seed))
        sub = R.host_subsets(None, n, R.subset_size(float(ms), n), T)[None]
    out, res = align_depth_batch(rel[None], met[None], None if mask is None else mask[None], float(ms), float(cap), subsets=sub)
    out, want = out.cpu().numpy()[0], g[f"ad_{name}_out"]
    assert out.shape == want.shape and out.dtype == want.dtype
    if name == "novalid":
        assert int(res.status[0]) == 1
        np.testing.assert_array_equal(out, met)
    else:
        assert int(res.status[0]) == 0
    np.testing.assert_allclose(out, want, rtol=R.COEF_RTOL, atol=0)


def test_non_finite_selected_sample_fails_the_frame(torch_gpu, golden):
    """A NaN in the relative depth (np.isinf keeps it) or -inf in the metric depth (it passes `< max_valid_depth`) reaches the estimator:
    scikit-learn raises, the reference returns the metric depth - status 2 here, for that frame only."""
    g = golden("g10_align.npz")
    rel, met = g["ad_nomask_rel"], g["ad_nomask_met"]
    rel_nan, met_ninf = rel.copy(), met.copy()
    picked = np.argwhere(_valid(rel, met, None, 400.0))
    rel_nan[tuple(picked[40])] = np.nan
    met_ninf[tuple(picked[900])] = -np.inf
    rels, mets = np.stack([rel, rel_nan, rel]), np.stack([met, met, met_ninf])
    out, res = align_depth_batch(rels, mets, None, 0.2, 400.0, seed=3)
    assert res.status.cpu().tolist() == [0, 2, 2]
    out = out.cpu().numpy()
    np.testing.assert_array_equal(out[1], mets[1])
    np.testing.assert_array_equal(out[2], mets[2])
    assert np.isnan(res.coef.cpu().numpy()[1:]).all() and res.best_trial.cpu().tolist()[1:] == [-1, -1]
    sel = ~np.isinf(rel)
    np.testing.assert_array_equal(out[0][sel], rel[sel] * res.coef.cpu().numpy()[0])
    assert (out[0][~sel] == 10000.0).all()


def test_batch_frames_equal_their_single_frame_calls(torch_gpu):
    """P = 3 frames of 48 x 64 with different valid counts, one of them empty: every frame equals its own single-frame call bit for
    bit (aligned map and every result field); an out-of-range subset index fails that frame alone."""
    torch = torch_gpu
    rs = np.random.RandomState(9)
    H, W = 48, 64
    rel = rs.uniform(0.5, 4.0, (3, H, W)).astype(np.float32)
    met = (3.1 * rel + 0.05 * rs.randn(3, H, W)).astype(np.float32)
    o = rs.rand(3, H, W) < 0.3
    met[o] = rs.uniform(0.1, 30.0, int(o.sum())).astype(np.float32)
    mask = rs.rand(3, H, W) < np.array([0.9, 0.4, 0.7])[:, None, None]
    mask[1] = False                                        # the empty frame
    rel[2][rs.rand(H, W) < 0.2] = np.inf
    counts = [int(_valid(rel[p_], met[p_], mask[p_], 400.0).sum()) for p_ in range(3)]
    assert counts[1] == 0 and counts[0] != counts[2]
    ms = [R.subset_size(0.2, c) for c in counts]
    sub = np.full((3, T, max(ms)), -1, np.int32)
    for p_ in (0, 2):
        sub[p_, :, :ms[p_]] = R.host_subsets(np.random.RandomState(p_), counts[p_], ms[p_], T)
    out, res = align_depth_batch(rel, met, mask, 0.2, 400.0, subsets=sub)
    assert res.status.cpu().tolist() == [0, 1, 0]
    for p_ in range(3):
        o1, r1 = align_depth_batch(rel[p_:p_ + 1], met[p_:p_ + 1], mask[p_:p_ + 1], 0.2, 400.0, subsets=sub[p_:p_ + 1])
        assert torch.equal(out[p_].view(torch.int32), o1[0].view(torch.int32))
        for k in RansacScale._fields:
            a, b = getattr(res, k)[p_:p_ + 1], getattr(r1, k)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (p_, k)
    bad = sub.copy()
    bad[2, 17, 3] = counts[2]                              # one past the end
    out2, res2 = align_depth_batch(rel, met, mask, 0.2, 400.0, subsets=bad)
    assert res2.status.cpu().tolist() == [0, 1, 2]
    assert torch.equal(out2[:2].view(torch.int32), out[:2].view(torch.int32))
    np.testing.assert_array_equal(out2[2].cpu().numpy(), met[2])
    neg = sub.copy()
    neg[0, 0, 0] = -1
    assert align_depth_batch(rel, met, mask, 0.2, 400.0, subsets=neg)[1].status.cpu().tolist() == [2, 1, 0]


def test_device_draw_subsets_are_distinct_and_keyed(torch_gpu):
    counts = np.array([5, 64, 4097], np.int64)
    a = ransac_subsets(counts, 0.2, T, seed=11).cpu().numpy()
    b = ransac_subsets(counts, 0.2, T, seed=12).cpu().numpy()
    assert a.shape == (3, T, R.subset_size(0.2, 4097)) and a.dtype == np.int32
    for p_, n in enumerate(counts):
        m = R.subset_size(0.2, int(n))
        rows = a[p_, :, :m]
        assert (rows >= 0).all() and (rows < n).all() and (a[p_, :, m:] == -1).all()
        assert all(len(set(r.tolist())) == m for r in rows)            # m DISTINCT indices per trial
        if n > 5:
            assert len({tuple(r) for r in rows.tolist()}) > T // 2       # trials differ
            assert (rows != b[p_, :, :m]).any(axis=1).sum() > T // 2     # seeds differ
    assert len({tuple(r) for r in a[0, :, :1].tolist()}) == 5            # n = 5, m = 1: every index is drawn by some trial
    # an integer min_samples, and a subset as large as the frame: a permutation of it
    full = ransac_subsets(np.array([64], np.int64), 64, 4, seed=1).cpu().numpy()[0]
    assert all(sorted(r.tolist()) == list(range(64)) for r in full)


def test_device_drawn_fit_equals_the_fit_fed_its_subsets(torch_gpu):
    torch = torch_gpu
    cases = [R.make_case(n, 0.3, 300 + n) for n in (5, 64, 4097)]
    xs, ys, counts, _ = _stack(cases, 0.2, 0)
    drawn = ransac_scale_batch(xs, ys, counts, 0.2, T, subsets=None, seed=5)
    again = ransac_scale_batch(xs, ys, counts, 0.2, T, subsets=None, seed=5)
    fed = ransac_scale_batch(xs, ys, counts, 0.2, T, subsets=ransac_subsets(counts, 0.2, T, seed=5))
    other = ransac_scale_batch(xs, ys, counts, 0.2, T, subsets=None, seed=6)
    assert drawn.status.cpu().tolist() == [0, 0, 0]
    for k in RansacScale._fields:
        assert torch.equal(getattr(drawn, k).view(torch.int32), getattr(again, k).view(torch.int32)), k     # run to run
        assert torch.equal(getattr(drawn, k).view(torch.int32), getattr(fed, k).view(torch.int32)), k
    assert not torch.equal(drawn.best_trial, other.best_trial) or not torch.equal(drawn.coef, other.coef)


def test_device_drawn_fit_lies_in_sklearns_own_spread(torch_gpu):
    """A clean synthetic frame (true scale 3.7, 30 % outliers): the coefficient of the device-drawn fit lies within the interval
    scikit-learn's own fit covers over 20 seeds on the same frame (computed here, on the CPU).  (The threshold is the MAD of a frame
    with uniform outliers, a wide band: both estimators sit near 3.80, not 3.7.)"""
    rs = np.random.RandomState(1)
    H, W = 48, 64
    rel = rs.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    met = (3.7 * rel + 0.05 * rs.randn(H, W)).astype(np.float32)
    o = rs.rand(H, W) < 0.3
    met[o] = rs.uniform(0.1, 30.0, int(o.sum())).astype(np.float32)
    coefs = [float(np.asarray(_sklearn(rel.reshape(-1), met.reshape(-1), 0.2, s).estimator_.coef_).reshape(-1)[0]) for s in range(20)]
    _, res = align_depth_batch(rel[None], met[None], None, 0.2, 400.0, seed=0)
    c = float(res.coef[0])
    print("device", c, "sklearn over 20 seeds", min(coefs), max(coefs))
    assert int(res.status[0]) == 0 and min(coefs) <= c <= max(coefs)


def test_unaligned_sample_rows(torch_gpu):
    """Sample buffers at a 4-byte (not 16-byte) aligned base, rows of a length that is no multiple of 4: the same results bit for bit."""
    torch = torch_gpu
    cases = [R.make_case(n, 0.3, 500 + n) for n in (4097, 257, 4001)]
    xs, ys, counts, sub = _stack(cases, 0.2, 3)
    assert xs.shape[1] % 4 == 1
    want = ransac_scale_batch(xs, ys, counts, 0.2, T, subsets=sub)
    dev = want.coef.device

    def shifted(a, dtype):
        buf = torch.empty(a.size + 1, dtype=dtype, device=dev)
        v = buf[1:].view(a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4
        return v

    got = ransac_scale_batch(shifted(xs, torch.float32), shifted(ys, torch.float32), counts, 0.2, T, subsets=shifted(sub, torch.int32))
    for k in RansacScale._fields:
        assert torch.equal(getattr(got, k).view(torch.int32), getattr(want, k).view(torch.int32)), k
    assert want.status.cpu().tolist() == [0, 0, 0]


def test_argument_refusals(torch_gpu):
    torch = torch_gpu
    from labelany3d_amd import _lib

    dev = torch.device("cuda", torch.cuda.current_device())
    P, n = 2, 64
    x = torch.ones((P, n), dtype=torch.float32, device=dev)
    cnt = torch.full((P,), n, dtype=torch.int64, device=dev)
    coef = torch.zeros(P, dtype=torch.float32, device=dev)
    ints = torch.zeros((4, P), dtype=torch.int32, device=dev)
    ws = torch.empty(int(_lib.lib.la3d_align_ransac_workspace_bytes(P, n, T)), dtype=torch.uint8, device=dev)

    def call(**over):
        a = _lib.AlignRansacArgs(struct_size=C.sizeof(_lib.AlignRansacArgs), P=P, n=n, relative_sel=x.data_ptr(), metric_sel=x.data_ptr(),
                                 counts=cnt.data_ptr(), min_samples=0.2, stop_probability=0.99, max_trials=T, m_cap=0, subsets=None, seed=0,
                                 coef=coef.data_ptr(), n_inliers=ints[0].data_ptr(), n_trials=ints[1].data_ptr(),
                                 best_trial=ints[2].data_ptr(), status=ints[3].data_ptr(), workspace=ws.data_ptr(), stream=None)
        for k, v in over.items():
            setattr(a, k, v)
        return _lib.lib.la3d_align_ransac_batch(C.byref(a))

    ERR_ARG, ERR_UNSUPPORTED = -1, -2
    assert call() == 0
    assert call(struct_size=C.sizeof(_lib.AlignRansacArgs) - 8) == ERR_ARG
    assert call(max_trials=0) == ERR_ARG
    assert call(min_samples=0.0) == ERR_ARG and call(min_samples=-0.5) == ERR_ARG and call(min_samples=2.5) == ERR_ARG
    assert call(coef=None) == ERR_ARG and call(relative_sel=x.data_ptr() + 2) == ERR_ARG
    assert call(n=_lib.ALIGN_RANSAC_MAX_N + 1) == ERR_UNSUPPORTED                     # refused before anything is launched
    assert call(max_trials=_lib.ALIGN_RANSAC_MAX_TRIALS + 1) == ERR_UNSUPPORTED
    assert call(P=65536) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    # the largest row the entry takes is at least 1 Mi samples
    assert _lib.ALIGN_RANSAC_MAX_N >= 1 << 20 and _lib.lib.la3d_align_ransac_workspace_bytes(1, 1 << 20, T) > 0
    with pytest.raises(ValueError):
        ransac_scale_batch(x, x, cnt[:1])
