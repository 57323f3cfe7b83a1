"""CPU tests of the differential slices and their checkers (oracle/campaigns/): what the committed seed lists cover, so that a later
edit cannot shrink the GPU slice unnoticed, and that every checker passes the oracle's own output and reports each planted error."""
import copy

import numpy as np
import pytest

from oracle import la3d_oracle as O
from oracle.campaigns import align_ransac as AR
from oracle.campaigns import annotations as A
from oracle.campaigns import aux as X
from oracle.campaigns import clouds as CL
from oracle.campaigns import engines as E
from oracle.campaigns import formats as FM
from oracle.campaigns import hull as HU
from oracle.campaigns import points as PT
from tests import campaign_slices as S


# ---------------------------------------------------------------------------------------------------------------------------------
# what the slices cover
# ---------------------------------------------------------------------------------------------------------------------------------
def _degenerate_ground(g):
    return g is not None and (np.all(g == [0, -1, 0, 1.0], axis=1).any() or (g[:, :3] == 0).all(1).any())


def test_slices_cover():
    assert len(S.ENGINE_SEEDS) >= 45 and len(S.ENGINE_TINY_SEEDS) >= 40
    assert all(10000 <= s < 14000 for s in S.ENGINE_SEEDS) and all(20000 <= s < 21500 for s in S.ENGINE_TINY_SEEDS)   # recorded in round 6
    reg = [E.make_case(s) for s in S.ENGINE_SEEDS]
    tiny = [E.make_case(s, tiny=True) for s in S.ENGINE_TINY_SEEDS]
    cases = reg + tiny
    assert set().union(*[set(c["mkind"]) for c in cases]) == set(range(15))               # every mask kind, 14 = polygons
    assert any(c["segs"] is not None for c in reg) and any(c["segs"] is not None for c in tiny)
    assert any(c["sidx"] is not None for c in reg) and any(c["sidx"] is not None for c in tiny)
    assert any(c["skew"] for c in reg)
    assert any(c["segs"] is not None and c["ground"] is not None for c in reg)
    assert any(c["sidx"] is not None and c["ground"] is not None for c in reg)

    def plane_mode(c):
        return "indexed" if c["image_index"] is not None else ("shared" if c["P"] == 1 else "private")

    def ground_mode(c):
        return "none" if c["ground"] is None else ("some" if np.isnan(c["ground"][:, 0]).any() else "all")

    assert {plane_mode(c) for c in reg} == {"shared", "private", "indexed"}
    assert {ground_mode(c) for c in reg} == {"none", "some", "all"}
    assert any(_degenerate_ground(c["ground"]) for c in reg)
    assert any(plane_mode(c) == "indexed" and ground_mode(c) == "some" for c in reg)
    # frames: untiled above 640 x 480, one above 1 Mpx (refused as run lengths / polygons), 640 x 480 itself, widths / heights off
    # the 32 x 8 tiles, tiny frames below one tile in either direction
    assert any(640 * 480 < c["H"] * c["W"] <= 1 << 20 for c in reg)
    assert any(c["H"] * c["W"] > 1 << 20 for c in reg)
    assert any((c["H"], c["W"]) == (480, 640) and c["B"] >= 16 for c in reg)
    assert any(c["W"] % 32 for c in reg) and any(c["H"] % 8 for c in reg)
    assert any(c["H"] < 8 and c["W"] < 32 for c in tiny) and any(c["H"] == 1 for c in tiny) and any(c["W"] == 1 for c in tiny)
    # batch sizes either side of the engines' thresholds (row / band engines up to 160, launch order above 256)
    assert any(c["B"] > 256 for c in reg) and any(160 < c["B"] <= 256 for c in reg) and any(c["B"] == 1 for c in reg)
    # an instance ill-conditioned for raw second moments
    for s in S.KAPPA_SEEDS:
        assert s in S.ENGINE_SEEDS
        _, rec, st, nv, kap = E.oracle_case(s)
        assert (kap[st == 0] > 2.0 ** 17).any(), s
    # the point clouds: both forms of the hull kernel, the subsample, both PCA solvers; ground and subsample modes
    pts = [PT.make_case(s) for s in S.POINT_SEEDS]
    sizes = {len(p) for c in pts for p in c["clouds"]}
    assert {0, 1, 2, 19, 20, 500, 501, 512, 513, 2048, 2049, 5000} <= sizes
    assert any(c["sidx"] is not None for c in pts) and any(c["sidx"] is None for c in pts)
    assert any(c["ground"] is not None and np.isnan(c["ground"][:, 0]).any() for c in pts)
    # annotations: every segmentation kind and several planes; aux: frames of one row / column
    anns = [A.make_case(s) for s in S.ANNOTATION_SEEDS]
    assert {"crowd", "none", "poly", "rle"} <= {k for c in anns for k in c["kinds"]} and any(c["P"] > 1 for c in anns)
    aux = [X.make_case(s) for s in S.AUX_SEEDS]
    assert any(c["poly"] is not None for c in aux) and any(c["depth_stats"] is not None for c in aux) and any(c["H"] == 1 for c in aux) \
        and any(c["W"] == 1 for c in aux)


def test_hull_slice_covers():
    """The convex-hull slice, from generator and oracle alone: every frame class, every refusal reason, both sides of the candidate
    and of the active-tile boundary, enough fitted instances in either mode and - a condition on the INPUTS, not a tolerance: a slice
    that misses it gets other seeds - at least 70 % of the hull-decided instances sharply decided (the reference alone: 79 % of the
    campaign's masks; the rest are parallel / perpendicular twins within 1e-9 of the minimum area)."""
    assert 55 <= len(S.HULL_SEEDS) <= 70 and all(70000 <= s < 70500 for s in S.HULL_SEEDS)
    cases = [HU.make_case(s) for s in S.HULL_SEEDS]
    refs = [HU.oracle_case(s) for s in S.HULL_SEEDS]
    full = [c for c in cases if c["full"]]
    samp = [c for c in cases if not c["full"]]
    frames = {(c["H"], c["W"]) for c in full}
    assert set(HU.TILED) | {HU.BIG, HU.ZERO_ROOM, HU.WIDE, HU.SMALL_OFF} <= frames and any(c["H"] < 10 for c in full)
    assert any(c["B"] <= 3 for c in full if (c["H"], c["W"]) == HU.BIG)
    sframes = {(c["H"], c["W"]) for c in samp}
    assert {HU.BIG, HU.ZERO_ROOM, HU.WIDE, HU.ODD_OFF, HU.SMALL_OFF, (96, 224), (240, 320), (100, 214)} <= sframes and any(c["H"] < 10 for c in samp)
    assert {c["B"] for c in cases} >= set(HU.BS) | {161, 300}
    for group in (full, samp):
        assert any(c["segs"] is not None for c in group) and any(c["skew"] for c in group)
        assert {"none", "some", "all"} == {"none" if c["ground"] is None else ("some" if np.isnan(c["ground"][:, 0]).any() else "all") for c in group}
        assert {"indexed", "shared", "private"} == {"indexed" if c["image_index"] is not None else ("shared" if c["P"] == 1 else "private") for c in group}
        assert any(_degenerate_ground(c["ground"]) for c in group)
    assert any(5 in c["dkind"] for c in full) and any(5 in c["dkind"] for c in samp)   # constant planes with zero / negative depths
    # every refusal reason; the candidate count on both sides of the hold, the active tiles on both sides of the room, per frame
    why, cands, tiles, early = set(), set(), set(), []
    redo = 0
    for c, ref in zip(full, [r for c, r in zip(cases, refs) if c["full"]]):
        Wp = HU.padded_width(c["W"])
        for n in range(c["B"]):
            ok, reason = HU.covered(c, n)
            why.add(reason)
            if reason in ("ground", "skew", "tiles"):                                # what the reference would have said of this instance
                g = c["ground"][n] if c["ground"] is not None and not np.isnan(c["ground"][n, 0]) else None
                early.append((reason, int(c["masks"][n].sum()), _degenerate_ground(None if g is None else g[None])))
            if reason in (None, "candidates"):
                cands.add(HU.candidate_count(c["masks"][n], c["depth"][HU.plane_of(c, n)]))
            if reason in (None, "tiles", "candidates") and c["fclass"] in ("tiled", "big"):
                tiles.add((c["H"], c["W"], HU.active_tiles(c["masks"][n]) - HU.tile_room(c["H"], Wp)))
            redo += bool(ok and ref.st[n] == 0 and ref.kap[n] > 2.0 ** 17)
        assert any(HU.applies(c, r) for r in HU.RUNS)
    assert why == set(HU.REASONS) | {None}
    assert {2047, 2048, 2049, 2050} <= cands
    for H, W in HU.TILED + [HU.BIG]:
        assert {(H, W, -1), (H, W, 0), (H, W, 1)} <= tiles, (H, W)
    # status 5 by ground row, skew or tiles comes before the reference's own statuses 1 / 2: empty masks, one-pixel masks and
    # degenerate ground rows among the instances refused for them
    assert {("ground", 0), ("skew", 0), ("ground", 1), ("tiles", 1)} <= {(reason, npx) for reason, npx, _ in early}
    assert sum(deg for _, _, deg in early) >= 5
    assert redo >= 3                                                                 # the second moments pass about the pivot
    # single columns and clouds of one to three points, fitted in full-mask mode
    kinds = {c["mkind"][n] for c in full for n in range(c["B"]) if HU.covered(c, n)[0]}
    assert {8, 10, 15, 16, 17, 18} <= kinds
    for mode in (True, False):
        cls = [k for c, ref in zip(cases, refs) if c["full"] == mode for k in ref.cls if k is not None]
        decided, tied, flat = cls.count("decided"), cls.count("tied"), cls.count("flat")
        assert len(cls) >= 150, (mode, len(cls))
        assert decided >= 0.7 * (decided + tied + flat), (mode, decided, tied, flat)
    st = np.concatenate([ref.st for ref in refs])
    cls = [k for ref in refs for k in ref.cls]
    assert (st == 1).sum() >= 5 and (st == 2).sum() >= 5 and cls.count("fallback") >= 5 and cls.count("tied") >= 5
    for r in HU.RUNS:
        assert sum(HU.applies(c, r) for c in cases) >= 5, r


def _frame_case(H, W, mask, depth=None, ground=None, skew=0.0):
    K = np.array([[[0.8 * W, skew, W / 2.0], [0, 0.8 * W, H / 2.0], [0, 0, 1]]])
    d = np.full((1, H, W), 2.0, np.float32) if depth is None else depth[None]
    return dict(H=H, W=W, B=1, P=1, K=K, depth=d, masks=mask[None], ground=ground, image_index=None, full=True)


def test_hull_coverage_rule_pins():
    """HU.covered against the figures the suite states (tests/test_gpu_hull_instances.py) and the limits of include/la3d.h."""
    rs = np.random.RandomState(1)
    for (H, W), room in (((96, 224), 28), ((128, 160), 40), ((200, 160), 85), ((240, 320), 220), ((64, 256), 0), ((96, 1056), 132)):
        assert HU.column_room(H, W) == HU.tile_room(H, W) == room
        for n, want in ((room, (True, None)), (room + 1, (False, "tiles"))):
            if n:
                assert HU.covered(_frame_case(H, W, HU.tile_rect_mask(rs, H, W, n)), 0) == want, (H, W, n)
    assert HU.covered(_frame_case(64, 256, np.zeros((64, 256), bool)), 0) == (True, None)      # (an empty mask has no tiles: status 1)
    # 640 x 480: the column arrays would fit behind 1040 of the 1200 tiles, but the tile list of four workgroups per CU holds 904,
    # and the compacted tiles with their range words fit up to 950
    assert HU.column_room(480, 640) == 1040 and HU.list_capacity(480, 640) == 904 and HU.tile_room(480, 640) == 904
    assert HU.covered(_frame_case(480, 640, HU.tile_rect_mask(rs, 480, 640, 904)), 0) == (True, None)
    assert HU.covered(_frame_case(480, 640, HU.tile_rect_mask(rs, 480, 640, 905)), 0) == (False, "tiles")
    # frames off the tiled path; the padded widths
    assert not HU.on_tiled_path(64, 96) and not HU.on_tiled_path(37, 64) and not HU.on_tiled_path(100, 214) and HU.on_tiled_path(100, 224)
    assert HU.tile_room(100, 224) == 31 and HU.tile_room(120, 256) == 56
    c = _frame_case(100, 214, HU.tile_rect_mask(rs, 100, 214, 5))
    assert HU.covered(c, 0, {}) == (True, None) and HU.covered(c, 0, dict(entry="ex_u8")) == (False, "frame")
    # ground row, skew, and their precedence over the mask
    m = HU.tile_rect_mask(rs, 96, 224, 3)
    assert HU.covered(_frame_case(96, 224, m, ground=np.array([[0.0, -1, 0, 1]])), 0) == (False, "ground")
    assert HU.covered(_frame_case(96, 224, m, ground=np.array([[np.nan, -1, 0, 1]])), 0) == (True, None)
    assert HU.covered(_frame_case(96, 224, m, skew=1e-3), 0) == (False, "skew")
    assert HU.covered(_frame_case(96, 224, np.zeros((96, 224), bool), skew=1e-3), 0) == (False, "skew")
    # candidates: one per column whose two ends coincide, two otherwise; 2048 are held
    H, W = 96, 1056
    one = np.zeros((H, W), bool); one[5, :] = True
    two = np.zeros((H, W), bool); two[5:7, :1025] = True
    d = np.full((H, W), 2.0, np.float32)
    assert HU.candidate_count(one, d) == 1056 and HU.candidate_count(two, d) == 1025
    assert HU.covered(_frame_case(H, W, two, d), 0) == (True, None)
    d2 = d.copy(); d2[6] = 3.0
    assert HU.candidate_count(two, d2) == 2050 and HU.covered(_frame_case(H, W, two, d2), 0) == (False, "candidates")
    d2[6, 0] = 2.0; d2[6, 1] = np.nan
    assert HU.candidate_count(two, d2) == 2048 and HU.covered(_frame_case(H, W, two, d2), 0) == (True, None)
    d2[5, 3] = -0.0; d2[6, 3] = 0.0
    assert HU.candidate_count(two, d2) == 2048                                       # (-0 and +0 are two floats)


def test_every_run_has_cases():
    """Every entry of RUNS / ANN_RUNS applies to some case of the slice (the polygon runs need polygon cases)."""
    reg = [E.make_case(s) for s in S.ENGINE_SEEDS]
    for r in E.RUNS + E.ANN_RUNS:
        assert any(E.applies(c, r) for c in reg), r
    assert dict(entry="ex_poly") in E.ANN_RUNS
    # the fused filter on polygons keeps enough instances to compare (its thresholds are drawn per case)
    kept = 0
    for c in reg:
        if c["segs"] is not None:
            _, size, flt = E.ex_params(c, "ex_poly")
            st = E.oracle_case(c["seed"])[2]
            keep = [O.keep_instance(O.mask_stats(m, flt["boundary_threshold"]), c["H"], False, flt["scale_threshold"]) for m in c["masks"]]
            kept += int((np.array(keep) & (st == 0)).sum())
    assert kept >= 50, kept


# ---------------------------------------------------------------------------------------------------------------------------------
# the checkers are sensitive: the oracle's own output passes, every planted error is reported
# ---------------------------------------------------------------------------------------------------------------------------------
def _engine_output(c, ref, r):
    """What a correct GPU run gives, from the oracle's result (aux: n_valid, n_masked and a resolved eigen-gap)."""
    rec, st, nv, kap = ref
    B = c["B"]
    aux = np.stack([np.zeros(B), nv, c["masks"].reshape(B, -1).sum(1), np.ones(B)], 1).astype(float)
    got = dict(boxes=rec.copy(), status=st.copy(), aux=aux)
    entry = r.get("entry")
    if entry in E.EX_ENTRIES:
        hint, size, flt = E.ex_params(c, entry)
        stats = None
        if flt is not None:
            stats = np.array([O.mask_stats(m, flt["boundary_threshold"]) for m in c["masks"]]).reshape(B, 4)
            keep = np.array([O.keep_instance(q, c["H"], entry == "ex_rle", flt["scale_threshold"]) for q in stats], bool)
            got["status"] = np.where(keep, st, 6).astype(np.int32)
            got["boxes"][~keep] = np.nan
        Kp = c["K"] if c["image_index"] is None else c["K"][c["image_index"]]
        with np.errstate(invalid="ignore", divide="ignore"):
            b2d = O.project_boxes(got["boxes"], Kp if (c["P"] > 1 or c["image_index"] is not None) else c["K"][0], size)
        b2d[got["status"] != 0] = np.nan
        got.update(boxes2d=b2d, stats=stats, flt=flt, size=size)
    return got


def _pick_center(rec, st, noise):
    """(instance, coordinate) of a fitted record whose centre coordinate is its largest entry of center / dims (a 1e-8 relative error
    there is 10 x the checker's 1e-9 of the scale) and whose reference noise is negligible."""
    best = None
    for n in np.flatnonzero(st == 0):
        j = int(np.argmax(np.abs(rec[n, :3])))
        share = abs(rec[n, j]) / max(1.0, np.abs(rec[n, :6]).max())
        if noise[n] < 1e-12 and (best is None or share > best[0]):
            best = (share, n, j)
    assert best is not None and best[0] > 0.5
    return best[1], best[2]


def _engine_case(poly):
    """The first (polygon) case of the slice with several fitted and some rejected instances."""
    for s in S.ENGINE_SEEDS:
        c = E.make_case(s)
        if (c["segs"] is not None) == poly and c["B"] * c["H"] * c["W"] < 2_000_000:
            ref = E.oracle_case(s)[1:]
            if (ref[1] == 0).sum() >= 3 and (ref[1] != 0).any():
                return c, ref
    raise AssertionError("no such case in the slice")


@pytest.mark.parametrize("r", [dict(), dict(entry="ex_u8"), dict(entry="ex_rle"), dict(entry="ex_poly")], ids=repr)
def test_engine_checker_sensitivity(r):
    from tests.test_gpu_parity import reference_axis_noise

    c, ref = _engine_case(poly=r.get("entry") == "ex_poly")
    good = _engine_output(c, ref, r)
    assert E.check_run(c, ref, r, good) == []
    st = good["status"]
    ok, bad = np.flatnonzero(st == 0), np.flatnonzero(st != 0)
    assert len(ok) and len(bad)
    i = ok[0]
    plants = {}
    g = copy.deepcopy(good); g["status"][i] = 3; plants["status"] = g
    g = copy.deepcopy(good); g["aux"][i, 1] += 1; plants["n_valid"] = g
    g = copy.deepcopy(good); g["aux"][i, 2] -= 1; plants["n_masked"] = g
    n, j = _pick_center(good["boxes"], st, reference_axis_noise(ref[3], good["aux"][:, 1], good["aux"][:, 3]))
    g = copy.deepcopy(good); g["boxes"][n, j] *= 1 + 1e-8; plants["center 1e-8"] = g
    g = copy.deepcopy(good); g["boxes"][bad[0]] = 0.0; plants["rejected not NaN"] = g
    if "boxes2d" in good:
        k = next(k for k in ok if np.isfinite(good["boxes2d"][k]).all())
        g = copy.deepcopy(good); g["boxes2d"][k, 1] += 1e-6; plants["2-D box 1e-6"] = g
    if good.get("stats") is not None:
        g = copy.deepcopy(good); g["stats"][ok[-1], 3] += 1; plants["filter statistic"] = g
    for name, g in plants.items():
        assert E.check_run(c, ref, r, g), f"planted error not reported: {name}"


def test_point_checker_sensitivity():
    from tests.test_gpu_parity import reference_axis_noise

    s = 0   # 33 clouds, fitted and rejected ones under both methods
    c = PT.make_case(s)
    ref = PT.oracle_case(s)[1]
    for method in PT.METHODS:
        rec, st, nv, kap = ref[method]
        good = (rec.copy(), st.copy(), np.stack([np.zeros(c["B"]), nv, np.zeros(c["B"]), np.ones(c["B"])], 1))
        assert PT.check_run(c, ref[method], method, {}, good) == []
        ok, bad = np.flatnonzero(st == 0), np.flatnonzero(st != 0)
        assert len(ok) and len(bad)
        n, j = _pick_center(rec, st, reference_axis_noise(kap, nv, np.ones(c["B"])) if method == "pca" else np.zeros(c["B"]))
        for name, (k, f) in dict(status=(1, lambda b, s_, a: s_.__setitem__(ok[0], 4)),
                                 n_valid=(2, lambda b, s_, a: a.__setitem__((ok[0], 1), a[ok[0], 1] + 1)),
                                 center=(0, lambda b, s_, a: b.__setitem__((n, j), b[n, j] * (1 + 1e-8))),
                                 dims=(0, lambda b, s_, a: b.__setitem__((n, 3), b[n, 3] + 1e-8 * np.abs(b[n, :6]).max())),
                                 height=(0, lambda b, s_, a: b.__setitem__((n, 4), b[n, 4] + 1e-8 * np.abs(b[n, :6]).max())),
                                 rejected=(0, lambda b, s_, a: b.__setitem__(bad[0], 0.0))).items():
            if method == "convex_hull" and name == "center":
                # (not a hull error the checker can see: two hull edges whose rectangles tie in area within 1e-9 give different,
                # equally right centres - the reference's choice between them is decided by its last bit - so a hull record is
                # held to its area and height there; the PCA records hold the centre)
                continue
            g = copy.deepcopy(good)
            f(*g)
            assert PT.check_run(c, ref[method], method, {}, g), f"{method}: planted error not reported: {name}"
        # the scalar drop-in's checker
        assert PT.check_scalar(c, ref[method], method, ok[0], (0, rec[ok[0]], np.array([0, nv[ok[0]], 0, 1.0]))) == []
        assert PT.check_scalar(c, ref[method], method, ok[0], (3, None, None))
        for k in ([j, 3, 4] if method == "pca" else [3, 4]):   # (hull: centre-only errors - see above)
            r1 = rec[n].copy(); r1[k] += 1e-8 * np.abs(r1[:6]).max()
            assert PT.check_scalar(c, ref[method], method, n, (0, r1, np.array([0, nv[n], 0, 1.0]))), (method, k)


def test_annotation_checker_sensitivity():
    s = next(s for s in S.ANNOTATION_SEEDS if (A.oracle_case(s)[1][1] == 0).sum() >= 3)
    c = A.make_case(s)
    ref = A.oracle_case(s)[1]
    rec, st, keep, keep_default, nv, kap, gap = ref
    want = np.flatnonzero(keep)
    outs = {("fit_annotations", False): ([c["anns"][i]["bbox"] for i in want], want, [c["anns"][i]["category_id"] for i in want], rec[want].copy(), st[want].copy())}
    for flt in (None, True, "thresholds"):
        k = np.array([m is not None for m in c["masks"]]) if flt is None else (keep_default if flt is True else keep)
        outs[("fit_annotations_all", flt)] = (np.where(k[:, None], rec, np.nan), np.where(k, st, 6).astype(np.int32))
    for call, good in outs.items():
        assert A.check_call(c, ref, call, good) == [], call
    b, stt = outs[("fit_annotations_all", None)]
    ok = np.flatnonzero((stt == 0) & (kap <= 2.0 ** 17) & (gap >= 1e-9))
    n = ok[np.argmax([abs(b[i, 2]) for i in ok])]
    for name, f in dict(status=lambda b, s_: s_.__setitem__(ok[0], 3),
                        center=lambda b, s_: b.__setitem__((n, 2), b[n, 2] * (1 + 1e-8)),
                        rejected=lambda b, s_: b.__setitem__(np.flatnonzero(stt != 0)[0], 0.0)).items():
        g = copy.deepcopy((b, stt))
        f(*g)
        assert A.check_call(c, ref, ("fit_annotations_all", None), g), f"planted error not reported: {name}"
    g = list(copy.deepcopy(outs[("fit_annotations", False)]))
    g[1] = g[1][:-1]
    assert A.check_call(c, ref, ("fit_annotations", False), tuple(g)), "a lost kept annotation is not reported"


def test_aux_checker_sensitivity():
    s = next(s for s in S.AUX_SEEDS if all(X.make_case(s)[k] is not None for k in ("rle", "poly", "depth_stats")))
    c = X.make_case(s)
    want = X.expected(c)
    assert X.check(c, want, want) == []
    fin = np.flatnonzero(np.isfinite(want["project_boxes"]).all(1))

    def plant(f):
        g = copy.deepcopy(want)
        f(g)
        return X.check(c, want, g)

    assert plant(lambda g: g["rle_decode"].__setitem__((0, 0, 0), ~g["rle_decode"][0, 0, 0]))
    assert plant(lambda g: g["mask_stats_rle"].__setitem__((0, 3), g["mask_stats_rle"][0, 3] + 1))
    assert plant(lambda g: g["poly_decode"].__setitem__((0, 0, 0), ~g["poly_decode"][0, 0, 0]))
    assert plant(lambda g: g["keep"][1].__setitem__(0, ~g["keep"][1][0]))
    assert plant(lambda g: g["project_boxes"].__setitem__((fin[0], 2), g["project_boxes"][fin[0], 2] + 1e-6))
    assert plant(lambda g: g["iou"].__setitem__((0, 0), g["iou"][0, 0] + 1e-9))
    assert plant(lambda g: g["median"][1].__setitem__(0, g["median"][1][0] + 1))
    assert plant(lambda g: g.__setitem__("align_apply", g["align_apply"] + 1))
    assert plant(lambda g: g["unproject"][0].__setitem__(np.isfinite(g["unproject"][0]).nonzero()[0][:1], 1e30))


def _hull_output(c, ref, r):
    """What a correct GPU run gives, from the oracle's result and the coverage rule."""
    st, why = HU.expected_status(c, ref, r)
    B = c["B"]
    nm = c["masks"].reshape(B, -1).sum(1).astype(float)
    boxes = np.where((st == 0)[:, None], ref.rec, np.nan)
    a3 = np.array([-float(len(ref.table[n][0])) if st[n] == 0 and ref.table[n] is not None else 1.0 for n in range(B)])
    aux = np.stack([ref.yaw, ref.nv.astype(float), nm, a3], 1)
    aux[st == 5] = [np.nan, 0.0, np.nan, np.nan]                                      # (refused before the mask was counted ...
    late = np.array([w == "candidates" for w in why])                                # ... or behind the fit stage: both counts)
    aux[late] = np.stack([np.full(B, np.nan), ref.nv.astype(float), nm, np.full(B, np.nan)], 1)[late]
    got = dict(boxes=boxes, status=st.copy(), aux=aux)
    if r.get("entry") in HU.EX_ENTRIES:
        hint, size, flt = E.ex_params(c, r["entry"])
        stats = None
        if flt is not None:
            stats = np.array([O.mask_stats(m, flt["boundary_threshold"]) for m in c["masks"]]).reshape(B, 4)
            keep = np.array([O.keep_instance(q, c["H"], True, flt["scale_threshold"]) for q in stats], bool)
            got["status"] = np.where(keep, st, 6).astype(np.int32)
            got["boxes"][~keep] = np.nan
            got["aux"][~keep] = np.stack([np.full(B, np.nan), np.zeros(B), nm, np.full(B, np.nan)], 1)[~keep]
        Kp = c["K"] if c["image_index"] is None else c["K"][c["image_index"]]
        with np.errstate(invalid="ignore", divide="ignore"):
            b2d = O.project_boxes(got["boxes"], Kp if (c["P"] > 1 or c["image_index"] is not None) else c["K"][0], size)
        b2d[got["status"] != 0] = np.nan
        got.update(boxes2d=b2d, stats=stats, flt=flt, size=size)
    return got


def _hull_case(want):
    """The first case of the slice in full-mask mode on the tiled path with a decided, a tied and a refused instance (want) ..."""
    for s in S.HULL_SEEDS:
        c = HU.make_case(s)
        if c["full"] and HU.on_tiled_path(c["H"], HU.padded_width(c["W"])):
            ref = HU.oracle_case(s)
            st, _ = HU.expected_status(c, ref, {})
            if all(k in [ref.cls[n] for n in np.flatnonzero(st == 0)] for k in want) and (st == 5).any():
                return c, ref, st
    raise AssertionError("no such case in the slice")


def test_hull_checker_passes_the_oracle_in_every_run():
    seen = set()
    for s in S.HULL_SEEDS[::4]:
        c, ref = HU.make_case(s), HU.oracle_case(s)
        for r in HU.RUNS:
            if HU.applies(c, r):
                assert HU.check_run(c, ref, r, _hull_output(c, ref, r)) == [], (s, r)
                seen.add(repr(r))
    assert len(seen) == len(HU.RUNS)


def test_hull_checker_sensitivity():
    c, ref, st = _hull_case(("decided", "tied"))
    good = _hull_output(c, ref, {})
    tally = HU.new_tally()
    assert HU.check_run(c, ref, {}, good, tally) == []
    assert tally["full"]["decided"] and tally["full"]["tied"] and sum(tally["full"]["refused"].values())
    ok = np.flatnonzero(st == 0)
    dec = next(n for n in ok if ref.cls[n] == "decided")
    tie = next(n for n in ok if ref.cls[n] == "tied")
    why = HU.expected_status(c, ref, {})[1]
    ref5 = int(next(n for n in np.flatnonzero(st == 5) if why[n] != "candidates"))   # refused before its mask was counted
    plants = {}
    # a decided record turned by a quarter: the same rectangle, length and width exchanged
    g = copy.deepcopy(good); g["boxes"][dec] = ref.box_under(dec, ref.yaw[dec] + np.pi / 2); g["aux"][dec, 0] += np.pi / 2; plants["decided, turned by 90 degrees"] = g
    # a PCA box where the call must refuse - with the status of a fit, and under the refusal's own status
    pts, gr = ref._pts.get(ref5, (None, None))
    pca = O.fit_instances(c["depth"][HU.plane_of(c, ref5)], c["masks"][ref5:ref5 + 1], c["K"][HU.plane_of(c, ref5)])[0][0] if pts is None else O.fit_points(pts, gr)[0]
    pca = np.where(np.isnan(pca), 1.0, pca)
    g = copy.deepcopy(good); g["boxes"][ref5] = pca; g["status"][ref5] = 0; g["aux"][ref5] = [0.1, 10, good["aux"][ref5, 2], 0.5]; plants["a PCA box in place of a refusal"] = g
    g = copy.deepcopy(good); g["boxes"][ref5] = pca; plants["a record under status 5"] = g
    g = copy.deepcopy(good); g["aux"][ref5, 0] = 0.3; plants["a yaw under status 5"] = g
    # a refusal in place of a fit
    g = copy.deepcopy(good); g["boxes"][dec] = np.nan; g["status"][dec] = 5; g["aux"][dec] = [np.nan, 0, np.nan, np.nan]; plants["a refusal in place of a fit"] = g
    # a tied record under a yaw that is no edge's (its own box under that yaw: consistent in itself, equal in area to 1e-4)
    g = copy.deepcopy(good); g["aux"][tie, 0] += 1e-2; g["boxes"][tie] = ref.box_under(tie, g["aux"][tie, 0]); plants["tied, the yaw of no edge"] = g
    g = copy.deepcopy(good); g["aux"][tie, 0] += 1e-2; plants["tied, the right box under a reported yaw that is no edge's"] = g
    g = copy.deepcopy(good); g["status"][ref5] = 1; plants["a refusal reported as the reference's empty cloud"] = g
    # ... and under a tied edge's yaw with another yaw's box
    twin = int(next(i for i in ref.near[tie] if HU._ang(ref.table[tie][0][i], ref.yaw[tie]) > 1e-6))
    g = copy.deepcopy(good); g["aux"][tie, 0] = ref.table[tie][0][twin]; plants["tied, the twin's yaw with the first edge's box"] = g
    # a column end lost: one extent of the footprint 1e-6 of the scale short
    scale = max(1.0, np.abs(ref.rec[dec, :6]).max())
    g = copy.deepcopy(good); g["boxes"][dec, 5] -= 1e-6 * scale; plants["decided, dx short by 1e-6"] = g
    g = copy.deepcopy(good); g["boxes"][dec, 3] -= 1e-6 * scale; plants["decided, dz short by 1e-6"] = g
    g = copy.deepcopy(good); g["boxes"][tie, 5] -= 1e-6 * max(1.0, np.abs(ref.rec[tie, :6]).max()); plants["tied, dx short by 1e-6"] = g
    g = copy.deepcopy(good); g["aux"][dec, 3] = 0.5; plants["decided, reported as a PCA fallback"] = g
    g = copy.deepcopy(good); g["aux"][dec, 1] += 1; plants["n_valid"] = g
    g = copy.deepcopy(good); g["aux"][dec, 2] -= 1; plants["n_masked"] = g
    g = copy.deepcopy(good); g["aux"][ref5, 2] = 1e9; plants["n_masked of a refused instance"] = g
    # refused by the ground row, the skew or the tiles: (n_valid, n_masked) = (0, NaN), not a count from somewhere else
    g = copy.deepcopy(good); g["aux"][ref5, 2] = c["masks"][ref5].sum(); plants["the mask count of an instance refused before the count"] = g
    g = copy.deepcopy(good); g["aux"][ref5, 1] = 3; plants["n_valid of an instance refused before the count"] = g
    for name, g in plants.items():
        assert HU.check_run(c, ref, {}, g), f"planted error not reported: {name}"
    # the tied record switched to its twin - that edge's yaw and the oracle's box under it - passes
    g = copy.deepcopy(good); g["aux"][tie, 0] = ref.table[tie][0][twin]; g["boxes"][tie] = ref.box_under(tie, ref.table[tie][0][twin])
    assert not np.allclose(g["boxes"][tie, 6:15], good["boxes"][tie, 6:15], atol=1e-6)
    assert HU.check_run(c, ref, {}, g) == []
    # pins: byte for byte
    assert HU.check_pin(good, copy.deepcopy(good)) == []
    g = copy.deepcopy(good); g["boxes"][dec, 0] = np.nextafter(g["boxes"][dec, 0], np.inf)
    assert HU.check_pin(good, g)


def test_hull_checker_counts_of_refused_instances():
    """include/la3d.h: an instance refused for its candidate count reports n_valid and n_masked exactly (it has been through the fit
    stage), every other refused instance n_valid 0 and n_masked NaN."""
    for s in S.HULL_SEEDS:
        c = HU.make_case(s)
        late = [n for n in range(c["B"]) if c["full"] and HU.covered(c, n)[1] == "candidates"]
        if late:
            break
    ref = HU.oracle_case(s)
    good = _hull_output(c, ref, {})
    assert HU.check_run(c, ref, {}, good) == []
    n = late[0]
    assert good["aux"][n, 1] > 1024 and good["aux"][n, 2] == c["masks"][n].sum() >= good["aux"][n, 1]
    plants = {}
    g = copy.deepcopy(good); g["aux"][n, 2] = np.nan; plants["n_masked NaN behind the fit stage"] = g
    g = copy.deepcopy(good); g["aux"][n, 1] = 0; plants["n_valid 0 behind the fit stage"] = g
    g = copy.deepcopy(good); g["aux"][n, 1:3] = [0, np.nan]; plants["the counts of an early refusal behind the fit stage"] = g
    g = copy.deepcopy(good); g["aux"][n, 2] += 1; plants["n_masked off by one"] = g
    g = copy.deepcopy(good); g["aux"][n, 1] -= 1; plants["n_valid off by one"] = g
    for name, g in plants.items():
        assert HU.check_run(c, ref, {}, g), f"planted error not reported: {name}"


def test_hull_checker_flat_rule_holds_the_footprint():
    """A flat record (the oracle's footprint has no area) whose GPU box has one fails, height and centre y right or not."""
    for s in S.HULL_SEEDS:
        ref = HU.oracle_case(s)
        flat = [i for i, k in enumerate(ref.cls) if k == "flat" and np.abs(ref.rec[i, 3:6]).max() > 0]
        if flat:
            break
    c, n = HU.make_case(s), flat[0]
    good = _hull_output(c, ref, {})
    assert HU.check_run(c, ref, {}, good) == []
    ext = np.abs(ref.rec[n, 3:6]).max()
    g = copy.deepcopy(good); g["boxes"][n, 3] = g["boxes"][n, 5] = ext
    assert any("footprint" in m for m in HU.check_run(c, ref, {}, g))


def test_hull_checker_flat_and_fallback_rules():
    """A fallback record is held to height and centre y whatever the hull did, and to the PCA rule where both sides took the PCA axis."""
    s = next(s for s in S.HULL_SEEDS if "fallback" in HU.oracle_case(s).cls and (not HU.make_case(s)["full"]))
    c, ref = HU.make_case(s), HU.oracle_case(s)
    good = _hull_output(c, ref, {})
    assert HU.check_run(c, ref, {}, good) == []
    n = ref.cls.index("fallback")
    scale = max(1.0, np.abs(ref.rec[n, :6]).max())
    g = copy.deepcopy(good); g["boxes"][n, 4] += 1e-8 * scale
    assert HU.check_run(c, ref, {}, g)
    g = copy.deepcopy(good); g["boxes"][n, 1] += 1e-8 * max(scale, abs(ref.rec[n, 1]))
    assert HU.check_run(c, ref, {}, g)
    g = copy.deepcopy(good); g["boxes"][n, 0] += 1e-6 * scale       # (both on the PCA axis, resolved gap: the centre is held too)
    assert HU.check_run(c, ref, {}, g)


# ---------------------------------------------------------------------------------------------------------------------------------
# the instance point clouds (oracle/campaigns/clouds.py)
# ---------------------------------------------------------------------------------------------------------------------------------
CLOUD_REQUIRED = (
    "uniform: band of 1024 words, all 65536 pixels set", "frames: band of 1024 words, all 65536 pixels set",
    "uniform: band of 1024 words, the last one short", "frames: rows padded to a pitch of 65536",
    "uniform: capacity band with fewer than 32 pixels over more than 512 words",
    "frames: capacity band with fewer than 32 pixels over more than 512 words",
    "band count from BAND_PIX", "trailing empty bands", "scan chunk 1", "scan chunk 2", "scan chunk 3", "B = 1025", "B = 1",
    "u8: both forms in one instance", "empty first", "empty last", "empty between", "all empty",
    "subsample: exactly 500 pixels", "subsample: exactly 501 pixels", "subsample: ranks outside the cloud", "subsample: repeated ranks",
    "subsample: the last rank", "C entry: more than 64 padding columns", "C entry: frame_width 1",
    "mixed: four sizes, one without an instance", "K shared, P > 1, image_index", "skew", "no skew", "u8 bytes 0", "u8 bytes 1", "u8 bytes 2")


def test_cloud_slice_covers():
    """The slice of the instance point clouds, from generator and oracle alone - conditions on the INPUTS: a slice that misses one gets
    other seeds.  Full bands of 1024 words (all set; the last word short; a sparse one whose select searches the whole table), a band
    count BAND_PIX dictates, scan chunks 1 / 2 / 3 with a ragged last run, both u8 forms within one instance, empty instances in every
    place, subsample mode under every run, the C entry's padding, mixed sizes, a shared K with an image_index - and the oracle's own
    rounding: within a tenth of the 1e-13 tolerance of a np.longdouble evaluation with K inverted in closed form."""
    assert 40 <= len(S.CLOUD_SEEDS) <= 56 and all(80000 <= s < 80500 for s in S.CLOUD_SEEDS) and len(set(S.CLOUD_SEEDS)) == len(S.CLOUD_SEEDS)
    cases = [CL.make_case(s) for s in S.CLOUD_SEEDS]
    have = set().union(*[CL.features(c) for c in cases])
    for name in CLOUD_REQUIRED:
        assert name in have, name
    assert "B = 2049" in have or "B = 2500" in have                                 # chunk 3 with a ragged last run
    assert any(c["B"] == 2049 and c["sizes"][0] == (33, 47) for c in cases)
    assert {sz for c in cases for sz in c["sizes"]} >= set(CL.TINY) | set(CL.CAPACITY) | {CL.BIG}
    assert all(c["B"] <= 3 for c in cases if set(c["sizes"]) & (set(CL.CAPACITY) | {CL.BIG}))
    assert all(max(c["sizes"]) <= (9, 40) or (c["sizes"][0], c["B"]) == ((33, 47), 2049) for c in cases if c["B"] > 300)
    for r in CL.RUNS:
        assert sum(CL.applies(c, r) for c in cases) >= 5, r
        if r:
            assert f"subsample: {r}" in have, r                                       # (an instance above 500 pixels with sample_idx)
    assert sum(int((c["counts"] > CL.NSAMPLE).sum()) for c in cases if c["sidx"] is not None) >= 10
    assert any(c["uniform"] for c in cases) and any(not c["uniform"] for c in cases)
    worst = 0.0
    for s, c in zip(S.CLOUD_SEEDS, cases):
        want = CL.oracle_case(s)
        for p in range(c["P"]):
            fin = np.isfinite(c["depth"][p]).reshape(-1)
            ld = CL.longdouble_cloud(c["depth"][p], c["K"][p])[fin]
            err = np.abs(want["clouds"]["f32"][p][fin] - ld) / (CL.TOL + CL.TOL * np.abs(ld))
            worst = max(worst, float(err.max()) if err.size else 0.0)
    assert worst <= 0.1, worst


def test_cloud_campaign_restates_the_band_split():
    """CL.bands against the library: la3d_instance_points_workspace_bytes is 4 B (bands + 1), sized for the frame's width and for its
    padded width - for every frame and batch size of the generator and a spread around the thresholds of cloud_bands."""
    from labelany3d_amd import _lib

    ws = _lib.lib.la3d_instance_points_workspace_bytes
    frames = CL.TINY + CL.CAPACITY + CL.SMALL + [CL.BIG, (1, 65535), (2, 32768), (2, 32769), (3, 21845), (3, 21846), (5, 65536), (257, 255),
                                                 (256, 256), (255, 257), (1024, 64), (1025, 64), (4, 7), (5, 7), (2000, 33)]
    for H, W in frames:
        for B in CL.BS + CL.LARGE_BS + [4, 127, 128, 129, 1024, 2048, 4096, 8191, 8192, 8193, 100000]:
            Wp = CL.padded_width(W)
            want = 4 * B * (max(CL.bands(B, H, W), CL.bands(B, H, Wp)) + 1) if Wp <= CL.BAND_PIX else 0
            assert ws(B, H, W) == want, (B, H, W)
    assert CL.bands(1, 3, 65536) == 3 and CL.bands(1, 4, 16384) == 1 and CL.bands(1, 480, 640) == 64 and CL.bands(2500, 9, 40) == 3
    assert CL.band_words(1, 1, 65536) == [1024] and CL.band_words(1, 2, 65535) == [1024, 1024] and max(CL.band_words(3, 480, 640)) == 80
    assert [CL.scan_chunk(B) for B in (1, 1024, 1025, 2048, 2049, 2500)] == [1, 1, 2, 2, 3, 3]
    assert set(CL.u8_forms(2, 1000, 1, 0)) == {"16", "general"} and set(CL.u8_forms(2, 1000, 1, 1)) == {"general"}


def test_cloud_campaign_restatements_agree():
    """The campaign's private copies of the suite's rules: the 16-bit quantisers (tests/depth16_cases.py), the ten standard masks and
    the cloud rule (tests/instance_points_cases.py) - two independent restatements each."""
    from tests import depth16_cases as D16
    from tests import instance_points_cases as IC

    rs = np.random.RandomState(3)
    d = np.concatenate([CL.special_plane(rs, 40, 70).reshape(-1), np.float32([6.55349, 6.5535, 6.55351, 70000.0, 1e-9, 6e-8, 65504.0, 65520.0, -0.0])])
    for dtype, scale in [("f16", 1.0)] + [("u16", s) for s in CL.SCALES]:
        q = CL.quantise(d, dtype, scale)
        np.testing.assert_array_equal(q, D16.quantise(d, dtype, scale))
        for hole in (True, False):
            np.testing.assert_array_equal(CL.upconvert(q, scale, hole), D16.upconvert(q, scale, hole))
    for H, W in IC.FRAMES:
        np.testing.assert_array_equal(CL.standard_masks(H, W, 2), IC.standard_masks(H, W, 2))
    seen = set()
    for s in S.CLOUD_SEEDS:
        c = CL.make_case(s)
        key = (c["sidx"] is not None, c["cfw"] < c["W"]) if c["uniform"] else None
        if key is None or key in seen or c["B"] > 40 or c["H"] * c["W"] > 70000:
            continue
        seen.add(key)
        want = CL.oracle_case(s)
        for name, kind in (("f32", "f32"), ("u16h", "u16h"), ("c_u8", "f32")):
            rule = IC.cloud_rule(np.stack(CL.value_planes(c, kind)), np.stack(c["masks"]), c["K"], c["img"], c["sidx"], want[name]["fw"])
            for a, b in zip(CL.packed(want[name], np.arange(c["B"])), rule):
                np.testing.assert_array_equal(a, b, err_msg=f"seed {s} {name}")
    assert len(seen) == 4


def _cloud_output(c, want, r):
    """The oracle's own output, arranged as a correct run's (the rows the clouds are cut from: the oracle's planes)."""
    name, kind = CL.variant(c, r)
    order = CL.run_order(c, r)
    pts, pix, off, cnt = CL.packed(want[name], order)
    cap = c["cap"] if r.get("capacity") else None
    st = np.zeros(c["B"], np.int32)
    if cap is not None:
        st = (off[1:] > cap).astype(np.int32)
        live = np.repeat(st == 0, np.diff(off))
        T = len(pts)
        pts = np.concatenate([np.where(live[:, None], pts, CL.SENT), np.full((64, 3), CL.SENT)])
        pix = np.concatenate([np.where(live, pix, int(CL.SENT)), np.full(64, int(CL.SENT))]).astype(np.int32)
        assert len(pts) == T + 64
    if r.get("out") == "f32":
        pts, pix = pts.astype(np.float32), None
    return dict(points=pts, pixels=pix, offsets=off, counts=cnt.astype(np.int32), status=st, order=order, rows=want["clouds"][kind], capacity=cap)


def test_cloud_checker_passes_the_oracle_in_every_run():
    seen = set()
    for s in S.CLOUD_SEEDS[::3]:
        c, want = CL.make_case(s), CL.oracle_case(s)
        default = _cloud_output(c, want, {}) if c["uniform"] else None
        for r in CL.RUNS:
            if CL.applies(c, r):
                assert CL.check_run(c, want, r, _cloud_output(c, want, r), default) == [], (s, r)
                seen.add(repr(r))
    assert len(seen) == len(CL.RUNS)


def _cloud_case():
    """A uniform case of the slice in subsample mode with a rank outside a cloud, a short capacity that leaves instances on both
    sides, and a C-entry frame width below W that leaves pixels."""
    for s in S.CLOUD_SEEDS:
        c = CL.make_case(s)
        if not (c["uniform"] and c["sidx"] is not None and c["cap"] is not None and c["cfw"] < c["W"] and 3 <= c["B"] <= 300):
            continue
        want = CL.oracle_case(s)
        off = CL.packed(want["f32"], np.arange(c["B"]))[2]
        if (want["f32"]["pixels"][0] is not None and any((p == -1).any() for p in want["f32"]["pixels"]) and off[1] <= c["cap"] and
                len(CL.packed(want["c_u8"], np.arange(c["B"]))[0]) > 2 and c["cfw"] > 1):
            return c, want
    raise AssertionError("no such case in the slice")


def test_cloud_checker_sensitivity():
    """Every planted error is reported, and - RULES taken out one at a time - every rule of check_run is the only one that reports
    some planted error: none of them is redundant."""
    c, want = _cloud_case()
    B = c["B"]
    default = _cloud_output(c, want, {})
    good = {k: _cloud_output(c, want, r) for k, r in dict(default={}, c_u8=dict(entry="c_u8"), cap=dict(capacity="short"), f32=dict(out="f32"),
                                                         bits=dict(entry="bits", frame_pad=True)).items()}
    runs = dict(default={}, c_u8=dict(entry="c_u8"), cap=dict(capacity="short"), f32=dict(out="f32"), bits=dict(entry="bits", frame_pad=True))
    for k, g in good.items():
        assert CL.check_run(c, want, runs[k], g, default) == [], k
    g0 = good["default"]
    off, pix = g0["offsets"], g0["pixels"]
    fin = np.flatnonzero(np.isfinite(g0["points"]).all(1) & (np.abs(g0["points"][:, 0]) > 1e-3))
    i = int(next(i for i in fin if i + 1 in fin and np.searchsorted(off, i, "right") == np.searchsorted(off, i + 1, "right")))   # two finite rows of one instance
    lost = int(np.flatnonzero(pix == -1)[0])                                          # the row of a rank outside its cloud
    plants = []                                                                       # (name, run, output, default, the one rule that sees it or None)

    def plant(name, run, f, only=None, dflt=default):
        g = copy.deepcopy(good[run])
        d2 = f(g)
        plants.append((name, run, g, dflt if d2 is None else d2, only))

    def swap(g):
        g["points"][[i, i + 1]] = g["points"][[i + 1, i]]; g["pixels"][[i, i + 1]] = g["pixels"][[i + 1, i]]

    def drop(g):
        n = int(np.searchsorted(off, i, "right") - 1)
        g["points"][i:off[n + 1] - 1] = g["points"][i + 1:off[n + 1]].copy(); g["pixels"][i:off[n + 1] - 1] = g["pixels"][i + 1:off[n + 1]].copy()

    def with_W(g):
        px = g["pixels"].astype(np.int64)
        g["pixels"][:] = np.where(px >= 0, px // c["cfw"] * c["W"] + px % c["cfw"], -1)

    def ulp(g):
        g["points"][i, 0] = np.nextafter(g["points"][i, 0], np.inf)

    def both_off(g):
        g["points"][i, 0] *= 1 + 1e-12
        g["rows"] = [r.copy() for r in g["rows"]]
        n = int(np.searchsorted(off, i, "right") - 1)
        g["rows"][int(c["img"][n])][pix[i], 0] *= 1 + 1e-12

    gk = good["cap"]
    dead = np.flatnonzero(np.repeat(gk["status"] == 1, np.diff(gk["offsets"])))
    assert len(dead) and (gk["status"] == 0).any()
    T = int(off[-1])
    plant("two neighbouring rows exchanged", "default", swap)
    plant("two neighbouring points exchanged, pixels in place", "default", lambda g: g["points"].__setitem__([i, i + 1], g["points"][[i + 1, i]]))
    plant("a row dropped and the rest shifted", "default", drop)
    plant("an offset off by one", "default", lambda g: g["offsets"].__setitem__(2, g["offsets"][2] + 1), "offsets")
    plant("a count off by one", "default", lambda g: g["counts"].__setitem__(1, g["counts"][1] + 1), "counts")
    plant("a pixel index computed with W where the frame width is smaller", "c_u8", with_W, "pixels")
    plant("one coordinate off by 1e-12 relative", "default", lambda g: g["points"].__setitem__((i, 0), g["points"][i, 0] * (1 + 1e-12)))
    plant("one coordinate off by one ulp", "default", ulp, "rows")
    plant("the cloud and unproject off by 1e-12 alike", "default", both_off, "oracle")
    plant("a NaN row written as zeros", "default", lambda g: g["points"].__setitem__(lost, 0.0))
    plant("a non-NaN row for a rank outside the cloud", "default", lambda g: g["points"].__setitem__(lost, g["points"][i]))
    plant("pixel 0 in place of -1", "default", lambda g: g["pixels"].__setitem__(lost, 0), "pixels")
    plant("status 0 on an instance beyond the capacity", "cap", lambda g: g["status"].__setitem__(int(np.flatnonzero(g["status"] == 1)[0]), 0), "status")
    plant("status 1 on an instance within the capacity", "cap", lambda g: g["status"].__setitem__(int(np.flatnonzero(g["status"] == 0)[0]), 1), "status")
    plant("a sentinel overwritten inside a status-1 range", "cap", lambda g: g["points"].__setitem__((dead[-1], 2), 1.0), "sentinel")
    plant("a pixel sentinel overwritten inside a status-1 range", "cap", lambda g: g["pixels"].__setitem__(dead[0], 5), "sentinel")
    plant("a write beyond offsets[-1]", "cap", lambda g: g["points"].__setitem__((T, 0), 0.0), "sentinel")
    plant("a write at the very end of the buffers", "cap", lambda g: g["pixels"].__setitem__(T + 63, -1), "sentinel")
    plant("a row too many", "default", lambda g: g.__setitem__("points", np.concatenate([g["points"], np.zeros((1, 3))])), "shape")
    plant("float32 output with pixels", "f32", lambda g: g.__setitem__("pixels", pix.copy()), "shape")
    plant("float32 output one float32 step off", "f32", lambda g: g["points"].__setitem__((i, 0), np.nextafter(g["points"][i, 0], np.float32(np.inf))))

    def other_default(g):
        d2 = copy.deepcopy(default); d2["points"][i, 0] *= 1 + 1e-6
        return d2

    plant("float32 output that is not the cast of the float64 run", "f32", other_default, "cast")
    plant("bit planes: rows that are not the default run's", "bits", other_default, "default")
    for name, run, g, dflt, only in plants:
        assert CL.check_run(c, want, runs[run], g, dflt), f"planted error not reported: {name}"
        if only is not None:
            assert CL.check_run(c, want, runs[run], g, dflt, rules=[k for k in CL.RULES if k != only]) == [], f"{name}: reported without the rule '{only}'"
    assert {only for *_, only in plants if only} == set(CL.RULES)
    # every message names its rows / instances and the field
    msg = CL.check_run(c, want, {}, plants[0][2], default)
    assert any("instance" in m and ("pixels" in m or "points" in m) for m in msg), msg


# ---------------------------------------------------------------------------------------------------------------------------------
# the format converters (oracle/campaigns/formats.py)
# ---------------------------------------------------------------------------------------------------------------------------------
_FRAMES_RUNS = [r for r in FM.RUNS if r["entry"] == "frames" or r.get("form") == "frames"]
FORMAT_REQUIRED = (
    [f"frame {h}x{w}" for h, w in FM.TINY + [FM.BIG] + list(FM.VEC2) + FM.GEN2 + [FM.LONG]] + [f"unpack {a}/{b}" for a, b in FM.UNPACK]
    + ["second trip: vector packer, f32", "second trip: vector packer, f16", "second trip: vector packer, bf16", "second trip: vector packer, u8",
       "second trip: general packer, u8", "second trip: general packer, f32", "second trip: general packer, f16", "second trip: general packer, bf16",
       "second trip: unpacker, quad form", "depth trips 2/2", "masks u8", "masks bool", "u8 bytes 0", "u8 bytes 1", "u8 bytes 2"]
    + [f"labels {t}" for t in FM.LABEL_TYPES] + [f"logits {t}" for t in FM.LOGIT_TYPES] + [f"threshold {t!r}" for t in FM.THRESHOLDS]
    + ["device base 1", "device base 5", "device base 16", "plane stride above H*W", "u8 plane stride: multiple of 16 bytes",
       "u8 plane stride: no multiple of 16 bytes", "u8 canvas pitch: multiple of 16 bytes", "u8 canvas pitch: no multiple of 16 bytes",
       "lowest data_ptr is not the first image's", "an image with a (0, H, W) stack and no ids", "ids outside the dtype's range", "absent ids",
       "repeated ids", "negative ids", "fit leg", "fit16 f16", "fit16 u16h", "fit16 u16n"]
    + [f"second trip at its smallest frame {h}x{w}: vector packer, {e}" for (h, w), e in (((129, 512), "f32"), ((258, 512), "f16"), ((258, 512), "bf16"), ((516, 512), "u8"))]
    + [f"broken: {b}" for b in FM.BROKEN] + [f"scale {s!r}" for s in FM.D16_SCALES]
    + [f"depth: {n}" for n in ("tie, even k (power-of-two scale)", "tie, odd k (power-of-two scale)", "below a tie (power-of-two scale)",
                               "above a tie (power-of-two scale)", "65535 units", "65535.5 units", "above 65535 units", "subnormal", "half a unit")]
    + [f"run {FM.run_name(r)}: one size" for r in FM.RUNS] + [f"run {FM.run_name(r)}: mixed sizes" for r in _FRAMES_RUNS + [r for r in FM.RUNS if r["entry"] == "depth16"]])


def test_format_slice_covers():
    """The slice of the format converters, from the generator's features alone - conditions on the INPUTS: every frame (the second-trip
    frames of both packers for every element kind, the hand-made MaskBits, the long depth frame), every element kind of every packer in
    a one-size and a mixed case, every threshold, each layout, host and device ids, each broken input, both depth kinds (every run
    unpacks uint16 planes with both hole settings), every planted depth value, a mixed-size and a one-size case of every frames run -
    and, from the oracle alone, the fit leg (all three 16-bit kinds): more than 200 instances, at least half of its instances have status 0 and an eigen-gap of at least 1e-6."""
    assert 40 <= len(S.FORMAT_SEEDS) <= 56 and all(90000 <= s < 90500 for s in S.FORMAT_SEEDS) and len(set(S.FORMAT_SEEDS)) == len(S.FORMAT_SEEDS)
    cases = [FM.make_case(s) for s in S.FORMAT_SEEDS]
    feats = [FM.features(c) for c in cases]
    have = set().union(*feats)
    for name in FORMAT_REQUIRED:
        assert name in have, name
    for kind in [f"labels {t}" for t in FM.LABEL_TYPES] + [f"logits {t}" for t in FM.LOGIT_TYPES] + ["masks u8", "masks bool"]:
        for size in ("one size", "mixed sizes"):
            assert any(kind in f and size in f and "class tiny" in f for f in feats), (kind, size)
    assert sum(c["sizes"].count(FM.BIG) for c in cases) >= 1 and all(c["sizes"].count(FM.BIG) <= 1 for c in cases)
    assert all(max(c["B"].values()) <= 2 for c in cases if c["fclass"] in ("vec2", "gen2"))
    assert all(c["packer_only"] == (c["fclass"] != "tiny") for c in cases)
    for c in cases:                                               # the fit leg stays off the packer-only frames and the broken inputs
        assert not ((c["packer_only"] or c["broken"]) and any(FM.applies(c, r) for r in FM.RUNS if r["entry"] == "fit")), c["seed"]
    n_all = n_good = 0
    for s, c in zip(S.FORMAT_SEEDS, cases):
        if FM.has_fit(c):
            _, st, _, _, gap = FM.oracle_case(s)["fit"]["f32"]
            n_all += len(st)
            n_good += int(((st == 0) & (gap >= 1e-6)).sum())
    assert n_all > 200 and 2 * n_good >= n_all, (n_good, n_all)


def test_format_campaign_restates_the_limits():
    """The trip counts the campaign's docstring claims for every second-trip frame, from its restated constants (64 chunks of 256 lanes,
    elements per 16-byte group, grid_for's 16384 workgroups) - and the restated plane layout against frames.frame_bits_offsets."""
    from labelany3d_amd.frames import frame_bits_offsets, frame_table

    assert (FM.LANES, FM.CHUNKS, FM.GROUP_BYTES, FM.GRID, FM.DEPTH_GROUP) == (256, 64, 16, 16384, 8)
    for (H, W), elem in FM.VEC2.items():
        for e in ("f32", "f16", "bf16", "u8"):
            groups = H * W // (16 // FM.ELEM_BYTES[e])
            assert FM.vec_form(H, W, W, e) and FM.pack_trips(H, W, W, e) == -(-groups // 16384), (H, W, e)
        assert H * W // (16 // FM.ELEM_BYTES[elem]) == 16512 and FM.pack_trips(H, W, W, elem) == 2
        assert FM.pack_trips(16384 * (16 // FM.ELEM_BYTES[elem]) // W, W, W, elem) == 1     # (exactly 16384 groups: one full trip)
    assert not FM.vec_form(516, 512, 512, "u8", base_bytes=5) and not FM.vec_form(129, 512, 512, "u8", stride_elems=129 * 512 + 3)
    assert FM.pack_trips(96, 224, 224, "f16") == 1 and FM.pack_trips(480, 640, 640, "u8") == 2 and FM.pack_trips(480, 640, 640, "f32") == 5
    (H, W), (H2, W2) = FM.GEN2
    assert not FM.vec_form(H, W, W, "u8") and (H * W + 31) // 32 == 16400 and (H * W) % 32 and FM.pack_trips(H, W, W, "u8") == 2
    assert not FM.vec_form(H2, W2, 512, "u8") and H2 * 512 // 32 == 16400 and FM.pack_trips(H2, W2, 512, "f32") == 2
    assert FM.pack_trips(1024, 500, 512, "u8") == 1
    assert FM.unpack_trips(129, 512) == 2 and FM.unpack_trips(128, 512) == 1 and 129 * 512 // 4 == 16512
    assert FM.depth_trips(1, *FM.LONG, 1) == (2, 2) and FM.depth_trips(1, 4194304, 1, 1) == (1, 1) and FM.depth_trips(1, 480, 640, 640) == (1, 1)
    for w_in, fw in FM.UNPACK:                                    # which of the hand-made planes take the quad form's two-word read
        two = fw % 4 == 0 and any(((v * w_in + u) & 31) > 28 for v in range(40) for u in range(0, fw, 4))
        assert two == ((w_in, fw) in [(53, 52), (54, 52), (37, 36)]), (w_in, fw)
    rs = np.random.RandomState(0)
    for _ in range(20):
        sizes = [FM.TINY[i] for i in rs.randint(0, len(FM.TINY), 5)] + [FM.BIG]
        ii = rs.randint(0, len(sizes), 17)
        a, b = FM.bits_offsets(sizes, ii), frame_bits_offsets(frame_table(sizes), ii)
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1] == b[1]


def test_format_logit_neighbours():
    """For every threshold and storage type the generator's "largest <= t" and "smallest > t" are adjacent bit patterns of the type that
    straddle np.float32(t) - decided in np.longdouble on exactly converted values."""
    L = np.longdouble

    def value(pat, T):                                            # the stored value, without the campaign's own conversion
        b, e, m = (32, 8, 23) if T == "f32" else (16, 5, 10) if T == "f16" else (16, 8, 7)
        pat = int(pat)
        sign, ex, man = pat >> (b - 1), (pat >> m) & ((1 << e) - 1), pat & ((1 << m) - 1)
        bias = (1 << (e - 1)) - 1
        if ex == (1 << e) - 1:
            return L("nan") if man else (L("-inf") if sign else L("inf"))
        mag = L(man) * L(2) ** (1 - bias - m) if ex == 0 else (L(1) + L(man) / L(1 << m)) * L(2) ** (ex - bias)
        return -mag if sign else mag

    for t in FM.THRESHOLDS:
        t32 = L(np.float32(t))
        for T in FM.LOGIT_TYPES:
            le, gt = FM.neighbours(t, T)
            assert int(FM.key_of(gt, T)) == int(FM.key_of(le, T)) + 1, (t, T)
            assert value(le, T) <= t32 < value(gt, T), (t, T, hex(int(le)), hex(int(gt)))
            for pat in (le, gt, *FM.specials(T)):                 # the campaign's conversion is the exact one
                with np.errstate(invalid="ignore"):               # (a signalling NaN among the specials)
                    v, w = value(pat, T), L(FM.to_f32(np.asarray([pat]), T)[0])
                assert (v != v and w != w) or v == w, (T, hex(int(pat)))
            if T == "f32":
                assert value(le, T) == t32
    assert FM.neighbours(0.1, "f16") == (0x2E66, 0x2E67) and FM.neighbours(7e4, "f16") == (0x7BFF, 0x7C00) and FM.neighbours(-0.0, "bf16") == (0, 1)
    # the planes mean their masks wherever no special value is sprinkled in, and hold the neighbours and the specials
    rs = np.random.RandomState(1)
    stack = rs.rand(3, 40, 50) < 0.5
    for T in FM.LOGIT_TYPES:
        for t in FM.THRESHOLDS:
            pat = FM.logit_planes(rs, stack, t, T)
            agree = (FM.logit_mask(pat, t, T) == stack).mean()
            assert 0.9 < agree < 1.0, (T, t, agree)
            assert set(FM.neighbours(t, T)) <= set(pat.reshape(-1).tolist()) and np.isnan(FM.to_f32(pat, T)).any()


def _format_output(c, want, r):
    """The oracle's own answer, laid out as a correct run's (run_gpu's dict)."""
    e, fam, lay = r["entry"], FM.family(r), c["lay"]
    if e == "fit":
        rec, st, nv, _, gap = want["fit"][r["depth"]]
        aux = np.stack([np.zeros(len(st)), nv.astype(float), want["area"][c["fit_src"]].astype(float), np.where(st == 0, gap, np.nan)], 1)
        return dict(boxes=rec.copy(), status=st.copy(), aux=aux, sent=None)
    if e == "depth16":
        dt, pad = r["dtype"], lay["d16_pad"]
        words, bufs = [], []
        for p, (h, w) in enumerate(c["sizes"]):
            g = np.zeros((h, FM.padded_width(w) if pad else w), np.uint16)
            g[:, :w] = want["d16"][dt]["words"][p].view(np.uint16)
            words.append(g)
        if c["uniform"] and c["fclass"] != "long":
            n_el = words[0].size
            ostride = n_el + lay["d16_extra"]
            obuf = np.full(c["P"] * ostride + 8, FM.SENT16, np.uint16)
            for p in range(c["P"]):
                obuf[p * ostride:p * ostride + n_el] = words[p].reshape(-1)
            bufs.append((obuf, ostride, n_el, c["P"]))
        values = {h: [v.copy() for v in want["d16"][dt]["values"][h]] if (dt == "u16" or h) else [] for h in (True, False)}
        return dict(words=words, values=values, bufs=bufs, pad=pad, sent=None)
    fam = fam or "masks"
    masks, B, img = want["masks"][fam], c["B"][fam], c["img"][fam]
    if e == "frames":
        device = r.get("layout") == "device" or r.get("ids") == "device"
        order = lay["perm"][fam] if r.get("layout") == "device" else np.arange(B)
        Hb, Wb = max(h for h, _ in c["sizes"]), max(FM.padded_width(w) for _, w in c["sizes"])
        if r.get("ids") == "device":
            stride = (Hb * Wb // 32 + 3) // 4 * 4
            offs, total = np.arange(B, dtype=np.int64) * stride, B * stride
        else:
            offs, total = FM.bits_offsets(c["sizes"], img[order])
        buf = np.full(max(total, 4) + 8, FM.SENT, np.uint32) if device else np.zeros(max(total, 4), np.uint32)
        area, ii, offs_out = want["area"][fam][order].copy(), img[order].copy(), offs.copy()
        broke = c["broken"] if (c["broken"] and fam == "masks" and r.get("layout") == "device") else None
        for i, n in enumerate(order):
            ww = FM.plane_words(masks[n], FM.padded_width(masks[n].shape[1]))
            if broke and broke[1] == i:
                area[i] = 0
                if broke[0] in FM.BROKEN[2:]:
                    if broke[0] == FM.BROKEN[2]:
                        ii[i] = c["P"] if i % 2 else -1
                    else:
                        offs_out[i] = -4 if broke[0] == FM.BROKEN[3] else offs[i] + 2
                    continue
                ww = np.zeros_like(ww)
            buf[offs[i]:offs[i] + len(ww)] = ww
        return dict(buf=buf, offsets=offs_out, image_index=ii.astype(np.int32), area=area.astype(np.int32), H=Hb, W=Wb, order=np.asarray(order),
                    sent=FM.SENT if device else None)
    H, fw = c["sizes"][0]
    W_st = c["w_in"] if e == "unpack" else (FM.padded_width(fw) if FM.uniform_pad(c, r) else fw)
    device = r.get("layout") == "device" or r.get("ids") == "device"
    nw = (H * W_st + 31) // 32
    buf = np.full((B, nw + (lay["out_pad"] if device else 0)), FM.SENT, np.uint32)
    for n in range(B):
        buf[n, :nw] = FM.plane_words(masks[n], W_st)
    got = dict(buf=buf, H=H, W=W_st, fw=fw, sent=FM.SENT if device else None, unpacked=np.stack(masks), stats={b: want["stats"][fam][b].copy() for b in (10, 3)})
    if fam == "labels":
        got.update(area=want["area"][fam].astype(np.int32), image_index=img.copy())
    return got


def test_format_checker_passes_the_oracle_in_every_run():
    seen = set()
    for s in S.FORMAT_SEEDS:
        c, want = FM.make_case(s), FM.oracle_case(s)
        default = {}
        for r in FM.RUNS:
            if FM.applies(c, r):
                got = _format_output(c, want, r)
                fam = FM.family(r)
                if fam is not None and fam not in default:
                    default[fam] = FM.decoded(c, r, got)
                assert FM.check_run(c, want, r, got, default.get(fam)) == [], (s, r)
                seen.add(FM.run_name(r))
    assert len(seen) == len(FM.RUNS)


def test_format_checker_sensitivity():
    """One planted error per rule: the rule, run alone through rules=, reports it, and without the rule (and the ones named beside it,
    which see the same words) the checker is silent: none of the rules is redundant, none is vacuous."""
    run = lambda **kw: next(r for r in FM.RUNS if all(r.get(k) == v for k, v in kw.items()))   # noqa: E731
    cases = [(FM.make_case(s), FM.oracle_case(s)) for s in S.FORMAT_SEEDS]
    plants = []

    def plant(name, rule, c, want, r, f, also=(), default=None):
        good = _format_output(c, want, r)
        assert FM.check_run(c, want, r, good, default) == [], name
        bad = copy.deepcopy(good)
        f(bad)
        plants.append((name, rule, also, c, want, r, bad, default))

    # a mixed-size masks case without a broken input whose first three planes hold pixels; a width that is no multiple of 32
    c, want = next((c, w) for c, w in cases if not c["uniform"] and not c["broken"] and c["B"]["masks"] >= 3 and (w["area"]["masks"][:3] > 0).all())
    r = run(src="masks", entry="frames", layout="device")
    g = _format_output(c, want, r)
    order, offs = g["order"], g["offsets"]
    nw = [h * FM.padded_width(w) // 32 for h, w in (c["sizes"][int(c["img"]["masks"][n])] for n in order)]
    i = int(np.argmax(nw))
    for name, at in (("first", offs[i]), ("a middle", offs[i] + nw[i] // 2), ("the last", offs[i] + nw[i] - 1)):
        plant(f"one bit of {name} word flipped", "words", c, want, r, lambda b, at=at: b["buf"].__setitem__(at, b["buf"][at] ^ np.uint32(1)))
    j = next(k for k, n in enumerate(order) if c["sizes"][int(c["img"]["masks"][n])][1] % 32)
    plant("a padding bit set", "padding", c, want, r, lambda b: b["buf"].__setitem__(offs[j] + nw[j] - 1, b["buf"][offs[j] + nw[j] - 1] | np.uint32(1 << 31)), also=("words",))
    plant("an area off by one", "area", c, want, r, lambda b: b["area"].__setitem__(1, b["area"][1] + 1))
    plant("a wrong plane offset", "layout", c, want, r, lambda b: b["offsets"].__setitem__(2, b["offsets"][2] + 4))
    plant("a sentinel touched behind the planes", "sentinel", c, want, r, lambda b: b["buf"].__setitem__(len(b["buf"]) - 1, 0))
    gap_at = next((int(offs[k] + nw[k]) for k in range(len(order)) if nw[k] % 4), None)
    if gap_at is not None:
        plant("a sentinel touched between two planes", "sentinel", c, want, r, lambda b: b["buf"].__setitem__(gap_at, 0))
    dflt = FM.decoded(c, run(src="masks", entry="frames", layout="host"), _format_output(c, want, run(src="masks", entry="frames", layout="host")))
    other = copy.deepcopy(dflt)
    other[int(order[i])][0, 0] ^= True
    plants.append(("planes that are not the first run's", "agree", (), c, want, r, g, other))
    # a one-size case: the uniform entries
    c, want = next((c, w) for c, w in cases if c["uniform"] and c["fclass"] == "tiny" and c["B"]["masks"] >= 2 and c["sizes"][0][0] > 4 and w["area"]["masks"].min() > 0)
    r = run(src="masks", entry="uniform", layout="device")
    plant("a sentinel touched behind a plane of out=", "sentinel", c, want, r, lambda b: b["buf"].__setitem__((1, b["buf"].shape[1] - 1), 7))
    plant("one pixel of the unpacked mask wrong", "roundtrip", c, want, r, lambda b: b["unpacked"].__setitem__((0, 1, 0), ~b["unpacked"][0, 1, 0]))
    plant("a boundary statistic off by one", "stats", c, want, r, lambda b: b["stats"][3].__setitem__((0, 3), b["stats"][3][0, 3] + 1))
    plant("a stored width that is not the padded one", "layout", c, want, r, lambda b: b.__setitem__("W", b["W"] + 32))
    # logits: the stored value next to the threshold, on the wrong side
    for c, want in cases:
        le = FM.neighbours(c["threshold"], c["logit_type"])[0]
        hit = [(p, np.argwhere(st == le)) for p, st in enumerate(c["logits"])]
        hit = [(p, a[0]) for p, a in hit if len(a)]
        if c["uniform"] and c["fclass"] == "tiny" and hit:
            p, (k, v, u) = hit[0]
            n = int(np.flatnonzero(c["img"]["logits"] == p)[k])
            r = run(src="logits", entry="uniform", layout="host", frame_pad=True)
            Wp = FM.padded_width(c["sizes"][0][1])
            assert not want["masks"]["logits"][n][v, u]           # (the largest value <= the threshold does not pass x > threshold)
            plant("the logit just below the threshold packed as set", "words", c, want, r,
                  lambda b, n=n, at=(v * Wp + u): b["buf"].__setitem__((n, at // 32), b["buf"][n, at // 32] | np.uint32(1 << (at % 32))))
            break
    else:
        raise AssertionError("no one-size case of the slice stores the value just below its threshold")
    # 16-bit depth: one wrong word; an exact tie rounded away from even
    c, want = next((c, w) for c, w in cases if "tie, even k (power-of-two scale)" in c["planted"])
    r = run(entry="depth16", dtype="u16")
    q = [c["depth"][p].astype(np.float64) / c["scale"] for p in range(c["P"])]
    p, (v, u) = next((p, a[0]) for p, a in ((p, np.argwhere((x % 2 == 0.5) & (x < 65535))) for p, x in enumerate(q)) if len(a))
    assert want["d16"]["u16"]["words"][p][v, u] == int(q[p][v, u] - 0.5)
    plant("an exact tie rounded away from even", "depth16", c, want, r, lambda b: b["words"][p].__setitem__((v, u), b["words"][p][v, u] + 1))
    plant("one 16-bit word wrong", "depth16", c, want, run(entry="depth16", dtype="f16"), lambda b: b["words"][0].__setitem__((0, 0), b["words"][0][0, 0] ^ 1))
    plant("an unpacked hole that is 0.0", "depth16", c, want, r, lambda b: b["values"][True][p].__setitem__((v, u), np.float32(0) if np.isnan(b["values"][True][p][v, u]) else np.float32("nan")))
    # the fit leg
    c, want, n = next((c, w, int(np.flatnonzero((w["fit"]["f32"][1] == 0) & (w["fit"]["f32"][4] > 1e-3))[0])) for c, w in cases
                      if FM.has_fit(c) and ((w["fit"]["f32"][1] == 0) & (w["fit"]["f32"][4] > 1e-3)).any() and (w["fit"]["f32"][1] != 0).any())
    r = run(entry="fit", form="frames", depth="f32")
    m = int(np.flatnonzero(want["fit"]["f32"][1] != 0)[0])

    def swap(b):
        b["status"][[n, m]] = b["status"][[m, n]]

    plant("two status values exchanged", "fit", c, want, r, swap)
    plant("a record off by 1e-6", "fit", c, want, r, lambda b: b["boxes"].__setitem__((n, 0), b["boxes"][n, 0] + 1e-6 * max(1.0, np.abs(b["boxes"][n, :6]).max())))
    plant("a zero eigen-gap reported for a decided record", "fit", c, want, r, lambda b: b["aux"].__setitem__((n, 3), 0.0))
    plant("a NaN eigen-gap reported for a decided record", "fit", c, want, r, lambda b: b["aux"].__setitem__((n, 3), np.nan))
    plant("n_valid off by one", "fit", c, want, r, lambda b: b["aux"].__setitem__((n, 1), b["aux"][n, 1] + 1))
    for name, rule, also, c, want, r, bad, default in plants:
        assert FM.check_run(c, want, r, bad, default, rules=[rule]), f"planted error not reported by '{rule}' alone: {name}"
        rest = [k for k in FM.RULES if k != rule and k not in also]
        assert FM.check_run(c, want, r, bad, default, rules=rest) == [], f"{name}: reported without the rule '{rule}'"
    assert {rule for _, rule, *_ in plants} == set(FM.RULES)


# ---------------------------------------------------------------------------------------------------------------------------------
# the batched RANSAC scale fit (oracle/campaigns/align_ransac.py)
# ---------------------------------------------------------------------------------------------------------------------------------
ALIGN_REQUIRED = tuple(
    [f"family {k}" for k in list(AR.R.FAMILIES) + AR.SPECIAL] + ["status 0", "status 1", "status 2"] + [f"n = {n}" for n in AR.SIZES] +
    [f"draw-only n = {n}" for n in AR.DRAW_ONLY] + ["segments 1", "segments 2", "segments 3", "segments 4", "segments >= 5"] +
    [f"P = {p}" for p in AR.PS] + [f"max_trials {t}" for t in AR.TRIALS] + [f"stop_probability {p}" for p in AR.STOPS] +
    [f"min_samples {k}" for k in AR.MIN_SAMPLES] +
    ["a frame with m > n", "a frame with m == n", "m_cap tight", "m_cap wide", "m_cap short", "a frame whose m exceeds m_cap", "-1 behind m",
     "garbage behind m", "median of y: the upper middle value differs", "median of y: the upper middle value is equal",
     "median of |y - med|: the upper middle value differs", "median of |y - med|: the upper middle value is equal", "thr == 0: fits",
     "thr == 0: fails", "a trial with k < 2", "a trial whose inlier y are all equal", "a subset with sum xx == 0", "trial limit 0",
     "trial limit infinite", "early stop", "all trials run", "undecided: score", "undecided: limit", "undecided: slope", "depth mask", "depth without mask",
     "depth status 0", "depth status 1", "depth status 2"] + [f"depth {h}x{w}" for h, w in AR.FRAMES_HW])


def _align_slice():
    return [(AR.make_case(s), AR.oracle_case(s)) for s in S.ALIGN_RANSAC_SEEDS]


def test_align_ransac_slice_covers():
    """The slice of the RANSAC scale fit, from generator and oracle alone - conditions on the inputs and on the oracle's own walk of the
    loop: a slice that misses one gets other seeds.  Every family, status, listed n, segment count, parameter kind, both medians'
    upper-middle branch, thr == 0 frames that fit and that fail, the scores' special values, sum xx == 0, both special trial limits,
    every run with enough cases - and at most 5 % of the frames undecided."""
    assert 40 <= len(S.ALIGN_RANSAC_SEEDS) <= 56 and len(S.ALIGN_RANSAC_SEEDS) % 6 == 0
    assert all(100000 <= s < 100500 for s in S.ALIGN_RANSAC_SEEDS) and len(set(S.ALIGN_RANSAC_SEEDS)) == len(S.ALIGN_RANSAC_SEEDS)
    cases = _align_slice()
    have = set().union(*[AR.features(c, w) for c, w in cases])
    for name in ALIGN_REQUIRED:
        assert name in have, name
    for r in AR.RUNS:
        assert sum(AR.applies(c, r) for c, _ in cases) >= 20, r
    tally = AR.new_tally()
    for c, w in cases:
        AR.tally_case(tally, c, w)
        assert all(c["T"] != 1024 or n <= 1025 for n in c["ns"]) and max(c["ns"]) <= 20000      # the CPU oracle stays in milliseconds
    assert tally["undecided"] >= 2 and AR.undecided_share(tally) <= AR.UNDECIDED_CAP, AR.tally_lines(tally)
    assert tally["thr0"] >= 20 and tally["thr0 fitted"] >= 5 and tally["thr0"] - tally["thr0 fitted"] >= 5


def test_align_ransac_undecided_cap_over_the_whole_range():
    """At most 5 % of the frames of seeds 100000 ... 100499 are undecided - from the oracle alone (the record of the campaign,
    profiles/align_ransac/fuzz_align_ransac.txt, states the same count)."""
    tally = AR.new_tally()
    for s in range(100000, 100500):
        c = AR.make_case(s)
        AR.tally_case(tally, c, AR.expected(c))
    print("\n".join(AR.tally_lines(tally)))
    assert tally["frames"] > 5000 and AR.undecided_share(tally) <= AR.UNDECIDED_CAP, AR.tally_lines(tally)
    assert tally["decided"] == 6906 and tally["undecided"] == 28      # the numbers of the committed record


def test_align_ransac_classes_come_from_the_rounding_bounds():
    """The three causes on hand-made steps: a quotient next to a float32 boundary, a trial limit next to an integer (but not where
    nom == denom bit for bit), and the score bound - zero for a zero-variance score, of the order eps k S_c / den otherwise."""
    a = np.float32(2.5)
    mid = (float(a) + float(np.nextafter(a, np.float32(3)))) / 2
    assert AR._other_slope(mid * (1 + 2.0 ** -42)) is not None and AR._other_slope(mid * (1 + 2.0 ** -38)) is None
    assert AR._other_slope(float(a)) is None and AR._other_slope(None) is None and AR._other_slope(0.0) is None
    other = AR._other_slope(mid * (1 - 2.0 ** -42))
    assert {float(other), float(np.float32(mid * (1 - 2.0 ** -42)))} == {float(a), float(np.nextafter(a, np.float32(3)))}
    x = np.float32([1, 2, 3, 4, 5, 6]); y = np.float32([2.5, 5.1, 7.4, 10.2, 12.4, 15.1])
    tr = []
    AR.R.ransac_scale(x, y, np.array([[0, 1], [2, 3]]), 2, 2, 0.99, trace=tr)
    ev = tr[0]
    tol = AR._score_tol(x, y, np.median(y), ev)
    k, den = ev["k"], ev["parts"]["den"]
    s_c = float(((y[ev["inl"]].astype(np.float64) - float(np.median(y))) ** 2).sum())
    assert 0 < tol < 100 * AR.EPS * k * s_c / den + 1e-6 * ev["parts"]["num"] / den and tol >= 2 * AR.EPS
    assert AR._score_tol(x, y, 0.0, dict(ev, parts=dict(num=0.0, den=0.0))) == 0.0
    ev2 = dict(ev, accepted=True, limit_q=3.0 * (1 + 1e-12), limit_same=False, s=None)
    assert ("limit", ev["t"], 3.0) in AR._ambiguities(x, y, np.median(y), [ev2], 100)
    assert not AR._ambiguities(x, y, np.median(y), [dict(ev2, limit_same=True)], 100)
    assert not AR._ambiguities(x, y, np.median(y), [dict(ev2, limit_q=3.001)], 100)
    assert not AR._ambiguities(x, y, np.median(y), [ev2], 2)                                     # an integer above max_trials


def _numpy_draw(counts, min_samples, T, seed):
    """Subsets of the form ransac_subsets documents, drawn with NumPy."""
    rs = np.random.RandomState(seed)
    ms = [AR.R.subset_size(min_samples, int(n)) if n > 0 else 0 for n in counts]
    ms = [m if 1 <= m <= n else 0 for m, n in zip(ms, counts)]
    sub = np.full((len(counts), T, max(ms + [1]) + 2), -1, np.int32)
    for p, (n, m) in enumerate(zip(counts, ms)):
        for t in range(T if m else 0):
            sub[p, t, :m] = rs.permutation(int(n))[:m]
    return sub


def _fields(frames):
    return {k: np.array([fw["res"][k] for fw in frames], np.float32 if k == "coef" else np.int32) for k in AR.FIELDS}


def _align_output(c, want, r):
    """The oracle's own output, arranged as a correct run's."""
    entry = r.get("entry")
    if entry is None:
        return _fields(want["frames"])
    if entry in ("seeded", "draw"):
        sub = _numpy_draw(c["counts"], c["min_samples"], c["T"], c["seed"])
        if entry == "draw":
            return dict(subsets=sub, extra=_numpy_draw(c["draw_extra"], c["min_samples"], AR.DRAW_ONLY_TRIALS, 1) if c["draw_extra"] else None)
        f = _fields([AR.frame_oracle(c["x"][p], c["y"][p], int(c["counts"][p]), c["n_cap"], sub[p], c["min_samples"], c["T"], c["stop"])
                     for p in range(c["P"])])
        return dict(drawn=f, fed=copy.deepcopy(f), subsets=sub)
    d, wd = c["depth"], want["depth"]
    g = _fields(wd["frames"])
    n = d["H"] * d["W"]
    rel_sel, met_sel, out = np.full((d["P"], n), -7.0, np.float32), np.full((d["P"], n), -7.0, np.float32), d["met"].copy()
    for p in range(d["P"]):
        rel_sel[p, :d["ns"][p]], met_sel[p, :d["ns"][p]] = wd["sel"][p]
        if g["status"][p] == 0:
            sel = d["mask"][p] if d["mask"] is not None else ~np.isinf(d["rel"][p])
            with np.errstate(over="ignore", invalid="ignore"):
                out[p] = np.where(sel, d["rel"][p] * g["coef"][p], AR.FILL)
    return dict(g, out=out, counts=np.array(d["ns"], np.int64), rel_sel=rel_sel, met_sel=met_sel)


def test_align_ransac_checker_passes_the_oracle_in_every_run():
    seen = set()
    for c, want in _align_slice()[::3]:
        default = _align_output(c, want, {})
        for r in AR.RUNS:
            if AR.applies(c, r):
                assert AR.check_run(c, want, r, _align_output(c, want, r), default, AR.new_tally()) == [], (c["seed"], r)
                seen.add(repr(r))
    assert len(seen) == len(AR.RUNS)


def _align_cases():
    """A case of the slice with two fitted frames of different results that ran more than one trial and a failed frame; a depth case
    with a fitted frame that leaves pixels unselected and a frame that was not fitted."""
    fit = depth = None
    for c, want in _align_slice():
        res = [fw["res"] for fw in want["frames"]]
        ok = [p for p, w in enumerate(res) if w["status"] == 0 and w["n_trials"] > 2 and 0 < w["best_trial"] and not want["frames"][p]["undecided"]]
        if fit is None and len(ok) >= 2 and c["ms"][ok[0]] >= 2 and any(w["status"] == 2 for w in res) and not AR._same_result(res[ok[0]], res[ok[1]]):
            fit = (c, want, ok[0], ok[1], next(p for p, w in enumerate(res) if w["status"] == 2))
        d = c["depth"]
        if depth is None and d is not None:
            st = [fw["res"]["status"] for fw in want["depth"]["frames"]]
            sel = d["mask"] if d["mask"] is not None else ~np.isinf(d["rel"])
            ok = [p for p in range(d["P"]) if st[p] == 0 and not sel[p].all() and sel[p].any()]
            if ok and any(s != 0 for s in st):
                depth = (c, want, ok[0], next(p for p in range(d["P"]) if st[p] != 0))
    assert fit is not None and depth is not None
    return fit, depth


def test_align_ransac_checker_sensitivity():
    """One planted fault at a time in a good result: the checker reports each."""
    (c, want, i, j, bad), (cd, wantd, pd_ok, pd_bad) = _align_cases()
    good = _align_output(c, want, {})
    assert AR.check_run(c, want, {}, good) == []

    def planted(f, r=None, base=good, case=(c, want), default=None):
        g = copy.deepcopy(base)
        f(g)
        return AR.check_run(case[0], case[1], r or {}, g, default)

    def two_ulp(g):
        g["coef"][i] = np.nextafter(np.nextafter(g["coef"][i], np.float32(np.inf)), np.float32(np.inf))

    def failed(g):
        g["status"][i], g["coef"][i], g["n_inliers"][i], g["n_trials"][i], g["best_trial"][i] = 2, np.nan, 0, 0, -1

    def fitted(g):
        for k in AR.FIELDS:
            g[k][bad] = g[k][i]

    def other_row(g):
        for k in AR.FIELDS:
            g[k][i] = g[k][j]

    for name, f in [("n_trials + 1", lambda g: g["n_trials"].__setitem__(i, g["n_trials"][i] + 1)),
                    ("n_trials - 1", lambda g: g["n_trials"].__setitem__(i, g["n_trials"][i] - 1)),
                    ("the next trial as best", lambda g: g["best_trial"].__setitem__(i, g["best_trial"][i] + 1)),
                    ("the previous trial as best", lambda g: g["best_trial"].__setitem__(i, g["best_trial"][i] - 1)),
                    ("n_inliers + 1", lambda g: g["n_inliers"].__setitem__(i, g["n_inliers"][i] + 1)),
                    ("n_inliers - 1", lambda g: g["n_inliers"].__setitem__(i, g["n_inliers"][i] - 1)),
                    ("coef two ulp off", two_ulp), ("status 0 -> 2", failed), ("status 2 -> 0", fitted),
                    ("a frame answered with another frame's row", other_row),
                    ("a finite coef on a failed frame", lambda g: g["coef"].__setitem__(bad, 1.0))]:
        assert planted(f), f"planted error not reported: {name}"
    one_ulp = lambda g: g["coef"].__setitem__(i, np.nextafter(g["coef"][i], np.float32(np.inf)))   # noqa: E731
    assert planted(one_ulp) == []                                                       # the adjacent float32 is the rule against the oracle ...
    for form in ("single", "again", "shifted"):
        assert planted(lambda g: None, dict(form=form), default=good) == []
        assert planted(one_ulp, dict(form=form), default=good), form                   # ... but not between two runs: bit for bit
    # an undecided frame: only the oracle's own walks pass
    cu, wu = next((c_, w_) for c_, w_ in _align_slice() if any(fw["undecided"] and len(fw["alts"]) > 1 for fw in w_["frames"]))
    pu = next(p for p, fw in enumerate(wu["frames"]) if fw["undecided"] and len(fw["alts"]) > 1)
    gu = _align_output(cu, wu, {})

    def walk(g, a):
        for k in AR.FIELDS:
            g[k][pu] = a[k]

    for a in wu["frames"][pu]["alts"]:
        assert planted(lambda g: walk(g, a), base=gu, case=(cu, wu)) == []
    assert planted(lambda g: g["n_trials"].__setitem__(pu, g["n_trials"][pu] + 3), base=gu, case=(cu, wu))
    assert planted(lambda g: walk(g, dict(wu["frames"][pu]["alts"][1], status=2)), base=gu, case=(cu, wu))
    # the draw
    r = dict(entry="draw")
    gd = _align_output(c, want, r)
    assert AR.check_run(c, want, r, gd) == []
    m, n = c["ms"][i], c["ns"][i]
    assert 2 <= m <= n

    def twice(g):
        g["subsets"][i, 3, 1] = g["subsets"][i, 3, 0]

    for name, f in [("an index drawn twice", twice), ("an index equal to n", lambda g: g["subsets"].__setitem__((i, 5, m - 1), n)),
                    ("a negative index", lambda g: g["subsets"].__setitem__((i, 0, 0), -1)),
                    ("an entry behind m that is not -1", lambda g: g["subsets"].__setitem__((i, 2, m), 0))]:
        assert planted(f, r, gd), f"planted error not reported: {name}"
    none = _numpy_draw([0, 5, 9], 7, 4, 0)                                              # no sample, m > n, m <= n
    assert (none[:2] == -1).all() and AR.check_draw([0, 5, 9], 7, none, 4) == []
    for p in (0, 1):
        none2 = none.copy()
        none2[p, 1, 0] = 0
        assert AR.check_draw([0, 5, 9], 7, none2, 4), "a row for a frame that cannot be drawn for"
    rs_ = dict(entry="seeded")
    gs = _align_output(c, want, rs_)
    assert AR.check_run(c, want, rs_, gs) == []
    assert planted(twice, rs_, gs)
    assert planted(lambda g: g["fed"]["coef"].__setitem__(i, np.nextafter(g["fed"]["coef"][i], np.float32(0))), rs_, gs)
    assert planted(lambda g: [g[k]["n_trials"].__setitem__(i, g[k]["n_trials"][i] + 1) for k in ("drawn", "fed")], rs_, gs)
    # the chain
    rc = dict(entry="chain")
    gc = _align_output(cd, wantd, rc)
    assert AR.check_run(cd, wantd, rc, gc) == []
    d = cd["depth"]
    sel = d["mask"][pd_ok] if d["mask"] is not None else ~np.isinf(d["rel"][pd_ok])
    off, on = tuple(np.argwhere(~sel)[0]), tuple(np.argwhere(sel & np.isfinite(d["rel"][pd_ok]))[0])

    def left_scaled(g):
        g["out"][pd_bad] = g["out"][pd_bad] * np.float32(2) + np.float32(1)

    for name, f in [("a wrong fill pixel", lambda g: g["out"].__setitem__((pd_ok,) + off, 0.0)),
                    ("a selected pixel one ulp off", lambda g: g["out"].__setitem__((pd_ok,) + on, np.nextafter(g["out"][(pd_ok,) + on], np.float32(np.inf)))),
                    ("a metric-depth frame left scaled", left_scaled),
                    ("a selection count off by one", lambda g: g["counts"].__setitem__(pd_ok, g["counts"][pd_ok] + 1)),
                    ("two selected samples exchanged", lambda g: g["rel_sel"].__setitem__((pd_ok, [0, 1]), g["rel_sel"][pd_ok, [1, 0]])),
                    ("n_trials + 1 in the chain", lambda g: g["n_trials"].__setitem__(pd_ok, g["n_trials"][pd_ok] + 1))]:
        if name.startswith("two selected") and (d["ns"][pd_ok] < 2 or wantd["depth"]["sel"][pd_ok][0][0] == wantd["depth"]["sel"][pd_ok][0][1]):
            continue
        assert planted(f, rc, gc, (cd, wantd)), f"planted error not reported: {name}"
