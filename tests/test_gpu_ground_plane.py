"""GPU tests of the ground plane from depth (include/la3d.h "ground plane: RANSAC plane fit"; kernels: labelany3d_amd/csrc/la3d_plane.hip):
``plane_select_batch`` / ``plane_ransac_batch`` / ``ground_planes`` against the NumPy restatement (tests/ground_plane_cases.py) - the
select and every trial decision EXACTLY, the reported plane against an ``eigh`` refit on the same inlier set to 1e-9 rad -, the seeded
draw against ``ransac_subsets``, reproducibility, and the rendered scene the feature exists for."""
import ctypes as C

import numpy as np
import pytest

from . import ground_plane_cases as G

pytestmark = pytest.mark.gpu

SENTINEL_F, SENTINEL_I = -777.25, -7
FAR = 400.0


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def _dev(a, dtype=None):
    import torch

    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return t if dtype is None else t.to(dtype)


# ---- select ---------------------------------------------------------------------------------------------------------------------
def _frames(P, H, W, seed):
    """depth with everything a depth map can hold: NaN, +-inf, 0, negatives, subnormals, the 10000.0 fill - and plain metres"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.3, 30.0, (P, H, W)).astype(np.float32)
    odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, 1e-42, G.FILL, FAR, np.nextafter(np.float32(FAR), np.float32(1e9))], np.float32)
    hit = rng.random((P, H, W)) < 0.35
    d[hit] = odd[rng.integers(0, len(odd), int(hit.sum()))]
    d[:, : max(1, H // 8)] = G.FILL                                   # the band the depth alignment leaves at the top
    K = np.stack([np.array([[500.0 + 7 * p, 0.3 * p, W / 2.0 + p], [0.0, 510.0 - 3 * p, H / 2.0 - p], [0.0, 0.0, 1.0]]) for p in range(P)])
    return d, K


def _candidates(la, P, H, W, seed):
    """(bool (P,H,W), MaskBits stored with a width padded to 32 and GARBAGE in the padding columns)"""
    import torch

    rng = np.random.default_rng(seed)
    Wp = (W + 31) // 32 * 32
    stored = rng.random((P, H, Wp)) < 0.6                             # columns >= W: set at random, never image
    words = np.packbits(stored.reshape(P, -1), axis=1, bitorder="little").view(np.int32)
    return stored[:, :, :W], la.MaskBits(torch.as_tensor(words, device="cuda"), H, Wp, W)


def _select_raw(la, depth, K, cand, step, near, far):
    """the C entry on buffers filled with sentinels"""
    import torch

    from labelany3d_amd import _lib

    P, H, W = depth.shape
    cap = (-(-H // step)) * (-(-W // step))
    pts = torch.full((P, cap, 3), SENTINEL_F, dtype=torch.float64, device="cuda")
    pix = torch.full((P, cap), SENTINEL_I, dtype=torch.int32, device="cuda")
    cnt = torch.full((P,), SENTINEL_I, dtype=torch.int64, device="cuda")
    ws = torch.empty(_lib.lib.la3d_plane_select_workspace_bytes(P, H, W, step), dtype=torch.uint8, device="cuda")
    a = _lib.PlaneSelectArgs(struct_size=C.sizeof(_lib.PlaneSelectArgs), P=P, H=H, W=W, step=step, k_stride=9 if K.shape[0] > 1 else 0,
                             near_depth=near, far_depth=far, depth=depth.data_ptr(), K=K.data_ptr(),
                             candidates=None if cand is None else cand.bits.data_ptr(), cand_plane_stride=0 if cand is None else cand.bits.shape[1],
                             cand_width=0 if cand is None else cand.W, points=pts.data_ptr(), pixel=pix.data_ptr(), counts=cnt.data_ptr(),
                             workspace=ws.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib.la3d_plane_select_batch(C.byref(a))
    assert rc == 0, _lib.lib.la3d_last_error()
    torch.cuda.synchronize()
    return pts, pix, cnt


@pytest.mark.parametrize("H,W,step,P,shared_k,with_cand", [(37, 53, 1, 3, False, True), (37, 53, 2, 3, True, False), (37, 53, 4, 3, False, True),
                                                           (48, 64, 1, 3, True, True), (48, 64, 2, 3, False, False), (48, 64, 4, 3, False, True),
                                                           (480, 640, 4, 2, False, True)])
def test_select_equals_the_restatement_and_unproject(la, H, W, step, P, shared_k, with_cand):
    depth, K = _frames(P, H, W, seed=H * 1000 + W + step)
    if shared_k:
        K = K[:1]
    cand_bool, cand = _candidates(la, P, H, W, seed=step) if with_cand else (None, None)
    d, k = _dev(depth), _dev(K.reshape(-1, 9))
    near = 0.5
    pts, pix, cnt = _select_raw(la, d, k, cand, step, near, FAR)
    ref_rows = la.unproject(d, K[0] if shared_k else K).reshape(P, H * W, 3).cpu().numpy()
    pts, pix, cnt = pts.cpu().numpy(), pix.cpu().numpy(), cnt.cpu().numpy()
    for p in range(P):
        want = G.select_ref(depth[p], None if cand_bool is None else cand_bool[p], step, near, FAR)
        assert cnt[p] == len(want) and 0 < len(want) < pix.shape[1], (p, cnt[p], len(want))
        assert np.array_equal(pix[p, :cnt[p]], want)
        assert np.array_equal(pts[p, :cnt[p]].view(np.int64), ref_rows[p][want].view(np.int64))                  # bit for bit
        assert (pix[p, cnt[p]:] == SENTINEL_I).all() and (pts[p, cnt[p]:] == SENTINEL_F).all()                   # not written
    # the Python entry: the same answer
    wp, wx, wc = la.plane_select_batch(d, K[0] if shared_k else K, cand, step=step, near=near, far=FAR)
    assert np.array_equal(wc.cpu().numpy(), cnt)
    for p in range(P):
        assert np.array_equal(wx[p, :cnt[p]].cpu().numpy(), pix[p, :cnt[p]])
        assert np.array_equal(wp[p, :cnt[p]].cpu().numpy().view(np.int64), pts[p, :cnt[p]].view(np.int64))


def test_select_defaults_keep_every_positive_finite_depth_and_an_empty_frame_counts_zero(la):
    depth, K = _frames(2, 37, 53, seed=5)
    depth[1] = np.nan
    _, pix, cnt = la.plane_select_batch(depth, K, step=3)
    cnt = cnt.cpu().numpy()
    want = G.select_ref(depth[0], None, 3)
    assert cnt[0] == len(want) and cnt[1] == 0 and np.array_equal(pix[0, :cnt[0]].cpu().numpy(), want)
    assert (depth[0].reshape(-1)[want] == G.FILL).any()                # without `far` the fill is a depth like any other


# ---- RANSAC ---------------------------------------------------------------------------------------------------------------------
FIELDS = ("plane", "k_trial", "n_inliers", "best_trial", "rms", "status", "inliers")


def _host(res):
    return {k: getattr(res, k).cpu().numpy() for k in FIELDS if getattr(res, k) is not None}


def _run(la, cases, min_inliers=3, subsets=True, seed=0, T=None):
    pts, counts, sub = G.stack(cases)
    res = la.plane_ransac_batch(_dev(pts), _dev(counts), threshold=G.THR_ABS, threshold_rel=G.THR_REL, max_trials=sub.shape[1] if T is None else T,
                                max_tilt=G.MAX_TILT, min_inliers=min_inliers, subsets=_dev(sub) if subsets else None, seed=seed, inliers=True)
    return _host(res), pts, counts


def _check(got, pts, counts, cases, min_inliers=3, tag=""):
    """status, best_trial, k_trial EXACT against the restatement; the reported plane against the eigh refit on the same inlier set;
    n_inliers, flags and rms recounted under the RETURNED numbers"""
    n = pts.shape[1]
    for p, c in enumerate(cases):
        want = G.expected(c, n, min_inliers)
        who = (tag, p, c["name"])
        assert got["status"][p] == want["status"], who
        assert got["best_trial"][p] == want["best_trial"] and got["k_trial"][p] == want["k_trial"], (who, got["best_trial"][p], want["best_trial"])
        if want["status"] != G.OK:
            assert np.isnan(got["plane"][p]).all() and np.isnan(got["rms"][p]) and got["n_inliers"][p] == 0 and not got["inliers"][p].any(), who
            continue
        assert want["gap"] >= 1e-3, who                                # (what the bounds below rest on: test_ground_plane_contract)
        plane = got["plane"][p]
        assert abs(np.linalg.norm(plane[:3]) - 1.0) <= 1e-15 and plane[1] <= 0, who
        err = G.angle(plane[:3], want["plane"][:3])
        assert err <= 1e-9, (who, err)
        assert abs(plane[3] - want["plane"][3]) <= 1e-9 * (1.0 + abs(want["plane"][3])), who
        flags, rms = G.recount_ref(c["points"][:c["count"]], plane, G.THR_ABS, G.THR_REL)
        assert got["n_inliers"][p] == flags.sum() and np.array_equal(got["inliers"][p, :c["count"]] != 0, flags), who
        assert not got["inliers"][p, c["count"]:].any(), who
        assert abs(got["rms"][p] - rms) <= 1e-9 * rms, (who, got["rms"][p], rms)


BATCHES = G.all_batches()


@pytest.mark.parametrize("tag", [t for t, _ in BATCHES])
def test_trial_decisions_are_exact_and_the_plane_is_the_refit(la, tag):
    cases = dict(BATCHES)[tag]
    got, pts, counts = _run(la, cases)
    _check(got, pts, counts, cases, tag=tag)


def test_min_inliers_above_the_best_k_fails_the_frame(la):
    cases = [g(G.SEG + 1, 65, 7) for g in G.GENERATORS]
    ks = sorted(G.expected(c)["k_trial"] for c in cases if G.expected(c)["status"] == G.OK)
    bar = ks[len(ks) // 2] + 1                                         # above the best k of some frames, not of others
    got, pts, counts = _run(la, cases, min_inliers=bar)
    _check(got, pts, counts, cases, min_inliers=bar, tag="min_inliers")
    st = got["status"]
    assert (st == G.OK).any() and sum(s == G.FAILED for s in st) > sum(G.expected(c)["status"] == G.FAILED for c in cases)


def test_seeded_draw_equals_the_call_fed_its_exported_subsets(la):
    T, seed = 65, 20261021
    cases = [G.tiny(0, T), G.tiny(2, T), G.tiny(3, T), G.tiny(4, T, 1), G.clean(300, T), G.wall(G.SEG + 1, T), G.non_finite(G.SEG, T)]
    pts, counts, _ = G.stack(cases)
    sub = la.ransac_subsets(_dev(counts), 3, T, seed)
    assert tuple(sub.shape) == (len(cases), T, 3)
    s = sub.cpu().numpy()
    for p, c in enumerate(counts):
        if c < 3:
            assert (s[p] == -1).all()
        else:
            assert ((s[p] >= 0) & (s[p] < c)).all() and all(len(set(r)) == 3 for r in s[p])
    kw = dict(threshold=G.THR_ABS, threshold_rel=G.THR_REL, max_trials=T, max_tilt=G.MAX_TILT, inliers=True)
    drawn = _host(la.plane_ransac_batch(_dev(pts), _dev(counts), seed=seed, **kw))
    fed = _host(la.plane_ransac_batch(_dev(pts), _dev(counts), subsets=sub, **kw))
    for k in FIELDS:
        assert drawn[k].tobytes() == fed[k].tobytes(), k
    assert list(drawn["status"][:5]) == [G.TOO_FEW, G.TOO_FEW, G.OK, G.OK, G.OK]
    other = _host(la.plane_ransac_batch(_dev(pts), _dev(counts), seed=seed + 1, **kw))
    assert other["best_trial"].tobytes() != drawn["best_trial"].tobytes() or other["plane"].tobytes() != drawn["plane"].tobytes()


def _ransac_raw(pts, counts, sub, out, ws, stream, T):
    from labelany3d_amd import _lib

    plane, ints, rms, flags = out
    P, n = pts.shape[:2]
    a = _lib.PlaneRansacArgs(struct_size=C.sizeof(_lib.PlaneRansacArgs), P=P, n=n, points=pts.data_ptr(), counts=counts.data_ptr(),
                             thr_abs=G.THR_ABS, thr_rel=G.THR_REL, cos2_tilt=G.cos2(G.MAX_TILT), max_trials=T, min_inliers=0,
                             subsets=sub.data_ptr(), seed=0, plane=plane.data_ptr(), k_trial=ints[0].data_ptr(), n_inliers=ints[1].data_ptr(),
                             best_trial=ints[2].data_ptr(), rms=rms.data_ptr(), status=ints[3].data_ptr(), inliers=flags.data_ptr(),
                             workspace=ws.data_ptr(), stream=stream.cuda_stream)
    rc = _lib.lib.la3d_plane_ransac_batch(C.byref(a))
    assert rc == 0, _lib.lib.la3d_last_error()


def test_runs_are_identical_alone_in_a_batch_and_replayed_from_a_graph(la):
    import torch

    from labelany3d_amd import _lib

    T = 64
    cases = [g(2 * G.SEG + 37, T, 11) for g in G.GENERATORS] + [G.clean(300, T, 3), G.wall(G.SEG - 1, T, 3)]
    first, pts, counts = _run(la, cases)
    second, _, _ = _run(la, cases)
    for k in FIELDS:
        assert first[k].tobytes() == second[k].tobytes(), k          # run to run
    _check(first, pts, counts, cases, tag="repro")
    n = pts.shape[1]
    for p in (0, 1, 5, len(cases) - 1):                               # a frame alone - in a row of the same capacity - and in the batch
        c = dict(cases[p], points=np.concatenate([cases[p]["points"], np.full((n - len(cases[p]["points"]), 3), np.nan)]))
        alone, _, _ = _run(la, [c])
        for k in FIELDS:
            assert alone[k][0].tobytes() == first[k][p].tobytes(), (p, k)
    # one captured call with a given workspace replays to the same bytes, on changed inputs too
    P = len(cases)
    _, _, sub = G.stack(cases)
    d_pts, d_cnt, d_sub = _dev(pts), _dev(counts), _dev(sub)
    out = (torch.empty((P, 4), dtype=torch.float64, device="cuda"), torch.empty((4, P), dtype=torch.int32, device="cuda"),
           torch.empty(P, dtype=torch.float64, device="cuda"), torch.empty((P, n), dtype=torch.uint8, device="cuda"))
    ws = torch.empty(_lib.lib.la3d_plane_ransac_workspace_bytes(P, n, T), dtype=torch.uint8, device="cuda")
    side, gr = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _ransac_raw(d_pts, d_cnt, d_sub, out, ws, side, T)          # (warm-up)
        side.synchronize()
        with torch.cuda.graph(gr, stream=side):
            _ransac_raw(d_pts, d_cnt, d_sub, out, ws, torch.cuda.current_stream(), T)
    order = list(range(1, P)) + [0]                                   # the second replay: the same frames in another order
    for perm in (list(range(P)), order):
        d_pts.copy_(_dev(pts[perm])); d_cnt.copy_(_dev(counts[perm])); d_sub.copy_(_dev(sub[perm]))
        for t in out:
            t.fill_(99)
        ws.fill_(0xA5)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        got = dict(plane=out[0], k_trial=out[1][0], n_inliers=out[1][1], best_trial=out[1][2], rms=out[2], status=out[1][3], inliers=out[3])
        for k in FIELDS:
            assert got[k].cpu().numpy().tobytes() == first[k][perm].tobytes(), k


# ---- the case the feature exists for --------------------------------------------------------------------------------------------
def test_a_box_on_the_floor_under_a_pitched_camera_is_fitted_upright(la):
    import torch

    s = G.scene()
    depth, mask, K = s["depth"], s["mask"], s["K"]
    d = _dev(np.stack([depth, np.full_like(depth, np.nan)]))          # image 1 has no depth at all: it stays "no ground"
    gp = la.ground_planes(d, K, step=4, far=100.0, threshold=0.005, max_tilt=0.8, seed=3)
    plane, status = gp.plane.cpu().numpy(), gp.status.cpu().numpy()
    assert status[0] == G.OK and status[1] == G.TOO_FEW and np.isnan(plane[1]).all()
    err = G.angle(plane[0, :3], s["normal"])
    print(f"ground plane: normal off by {err:.3e} rad, d {plane[0, 3]:.7f}, {int(gp.n_inliers[0])} inliers, rms {float(gp.rms[0]):.2e}")
    assert err <= 1e-4 and plane[0, 1] < 0 and abs(plane[0, 3] - s["d"]) <= 1e-3
    ii = torch.zeros(1, dtype=torch.int32, device="cuda")
    ground = gp.for_instances(ii)
    assert ground.is_cuda and ground.dtype == torch.float64 and tuple(ground.shape) == (1, 4)
    assert np.isnan(gp.for_instances([1, 0, 1]).cpu().numpy()[[0, 2]]).all()
    masks = _dev(mask[None].astype(np.uint8))
    boxes, st, _ = la.fit_instances(d, masks, K, ground=ground, image_index=ii)
    via_host, st_h, _ = la.fit_instances(d, masks, K, ground=plane[[0]], image_index=ii)
    flat, st_f, _ = la.fit_instances(d, masks, K, ground=None, image_index=ii)
    assert int(st[0]) == 0 and int(st_h[0]) == 0 and int(st_f[0]) == 0
    assert boxes.cpu().numpy().tobytes() == via_host.cpu().numpy().tobytes()
    upright, tilted = float(boxes[0, 4]), float(flat[0, 4])           # dimension = [dz, dy, dx]: the vertical one
    print(f"box height {s['box_height']}: with the plane {upright:.4f}, without {tilted:.4f}")
    assert abs(upright - s["box_height"]) <= 0.02 * s["box_height"]
    assert tilted > 1.10 * s["box_height"]
