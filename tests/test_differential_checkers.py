"""CPU tests of the differential slices and their checkers (oracle/campaigns/): what the committed seed lists cover, so that a later
edit cannot shrink the GPU slice unnoticed, and that every checker passes the oracle's own output and reports each planted error."""
import copy

import numpy as np
import pytest

from oracle import la3d_oracle as O
from oracle.campaigns import annotations as A
from oracle.campaigns import aux as X
from oracle.campaigns import engines as E
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
