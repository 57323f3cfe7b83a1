"""Randomised differential campaign of the path's other entries - everything either side of the box fit: case generator, the
reference expressions, GPU runs and the checker.  profiles/r06/fuzz_aux.py drives it at scale; tests/test_gpu_differential.py
runs a committed slice of its seeds.

Per case (random frame sizes incl. widths that are no multiple of 32 / 4, heights no multiple of 8):
  unproject     la3d_unproject / la3d_unproject_batch (reference src/util.py:52-75): depth with NaN / inf / zero / negative pixels, K with
                and without skew, per-frame K, R / t given or not, f64 and f32 output                     -> 1e-12 of the scale (f64)
  run lengths   la3d_rle_decode, la3d_mask_stats_rle, la3d_mask_stats on the decoded planes: uncompressed lists and the compressed
                string form, masks of every kind of the engine campaign                                   -> bit for bit / integer for integer
  polygons      la3d_poly_decode, la3d_mask_stats_poly against oracle/poly_oracle.py (the cv2.fillPoly restatement) -> bit for bit
  filters       keep_instances for both branches of the reference's rule (src/util.py:375)               -> the same decisions
  consumers     la3d_project_boxes (K shared / per box / indexed; corners behind the camera, on its plane) and la3d_iou_matrix
                (degenerate and disjoint boxes) against oracle project_boxes / iou2d_matrix               -> 1e-12
  depth stats   la3d_masked_ratio_median against np.median of the float32 ratios (ties, odd / even counts, 0/0, x/0), the depth-alignment
                selection (one frame and batched) and scatter against the reference's NumPy expressions (depth.py:67-90) -> bit for bit
  matcher       la3d_unproject_matches against the reference's expressions (src/matching/matcher.py:70-91)  -> 1e-12
make_case draws every input of a case, expected() computes what the reference computes, run_gpu() what the library computes, in
the same layout, and check() compares the two.  The oracle is test infrastructure: it is the checker here."""
import numpy as np

from oracle.campaigns import engines as FE

COUNTS = ("unproject", "rle", "poly", "stats", "keep", "project", "iou", "median", "align", "matches")


def rand_rot(rs):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    return q * np.sign(np.linalg.det(q))


def make_case(seed):
    """Every input of one case, drawn in the order the campaign has always drawn them (its records describe these cases)."""
    from oracle import la3d_oracle as O

    rs = np.random.RandomState(seed)
    H = int(rs.choice([1, 2, 7, 8, 16, 37, 64, 120, 240, 375, 480]))
    W = int(rs.choice([1, 3, 4, 31, 32, 33, 64, 100, 250, 333, 427, 640]))
    c = dict(seed=seed, H=H, W=W)
    # ---- unproject ----
    Pn = int(rs.choice([1, 1, 2, 5]))
    depth = np.stack([FE.one_plane(rs, H, W) for _ in range(Pn)])
    K = np.zeros((Pn, 3, 3))
    for p in range(Pn):
        f = rs.uniform(0.4, 3.0) * max(W, 8)
        K[p] = [[f, rs.uniform(-5, 5) * (rs.rand() < 0.3), W / 2 + rs.uniform(-0.3, 0.3) * W], [0, f * rs.uniform(0.8, 1.25), H / 2 + rs.uniform(-0.3, 0.3) * H], [0, 0, 1]]
    R = rand_rot(rs) if rs.rand() < 0.5 else None
    t = rs.randn(3) * 3 if rs.rand() < 0.5 else None
    c.update(depth=depth, K=K, R=R, t=t)
    # ---- run lengths / mask statistics / filters ----
    c["rle"] = c["poly"] = None
    if H >= 8 and W >= 32:
        B = int(rs.choice([1, 3, 17, 40]))
        masks = np.stack([FE.one_mask(rs, H, W) for _ in range(B)])
        rles = [O.rle_encode(m) for m in masks]
        if rs.rand() < 0.5:   # the compressed string form of the annotation files
            rles = [dict(size=r["size"], counts=(O.rle_to_string(r["counts"]) if rs.rand() < 0.7 else r["counts"])) for r in rles]
        bt = int(rs.choice([10, 10, 1, 3, 25]))
        u8_value = int(rs.choice([1, 255]))
        keep_thr = [int(rs.choice([100, 1, 1000])) for _ in (True, False)]   # scale thresholds of the two branches (from_rle True, False)
        c["rle"] = dict(masks=masks, rles=rles, bt=bt, u8_value=u8_value, keep_thr=keep_thr)
        # ---- polygons ----
        if H * W <= 120 * 333:
            Bp = int(rs.choice([1, 4, 12]))
            segs, pm = [], []
            for _ in range(Bp):
                m, seg = FE.one_polygon_mask(rs, H, W)
                segs.append(seg); pm.append(m)
            c["poly"] = dict(segs=segs, masks=np.stack(pm))
    # ---- consumers ----
    Bb = int(rs.choice([1, 5, 64, 300]))
    rec = rs.randn(Bb, 39) * 3
    rec[:, 15:] = (rs.randn(Bb, 8, 3) * [2, 1, 2] + [0, 0, rs.uniform(-1, 12)]).reshape(Bb, 24)
    if rs.rand() < 0.3:
        rec[rs.randint(Bb), 17] = 0.0        # a corner on the camera plane: division by zero, as in the reference
    if rs.rand() < 0.2:
        rec[rs.randint(Bb)] = np.nan         # a rejected box
    size = (int(rs.choice([640, 500, 427])), int(rs.choice([480, 375, 640])))
    kk = rs.randint(0, 3)
    Kb = K[0] if kk == 0 else np.stack([K[0] * [[rs.uniform(0.5, 2)], [rs.uniform(0.5, 2)], [1]] for _ in range(Bb)])
    ii = None
    if kk == 2:
        ii = rs.randint(0, Bb, Bb).astype(np.int32)
    n0, n1 = int(rs.choice([1, 7, 60])), int(rs.choice([1, 9, 80]))
    b0 = np.sort(rs.uniform(0, 640, (n0, 2, 2)), 1).reshape(n0, 4)[:, [0, 2, 1, 3]]
    b1 = np.sort(rs.uniform(0, 640, (n1, 2, 2)), 1).reshape(n1, 4)[:, [0, 2, 1, 3]]
    if rs.rand() < 0.5:
        b1[0] = b0[0]                        # identical boxes
        b1[-1, 2:] = b1[-1, :2]              # an empty box
    c.update(rec=rec, size=size, Kb=Kb, ii=ii, b0=b0, b1=b1)
    # ---- masked depth-ratio median (src/util.py:476-486), depth-alignment selection / scatter (depth.py:67-90), matcher ----
    c["depth_stats"] = None
    if H >= 2 and W >= 4:
        Bm = int(rs.choice([1, 3, 9]))
        num = np.stack([FE.one_plane(rs, H, W) for _ in range(Bm)])
        den = np.stack([FE.one_plane(rs, H, W) for _ in range(Bm)])
        if rs.rand() < 0.4:   # heavy ties: a handful of distinct ratios
            num = np.round(num).astype(np.float32); den = (np.round(np.abs(den)) + 1).astype(np.float32)
        ma = rs.rand(Bm, H, W) < 10 ** rs.uniform(-3, 0)
        mb = rs.rand(Bm, H, W) < rs.uniform(0.2, 1.0) if rs.rand() < 0.7 else None
        rel, met = num[0].copy(), np.abs(den[0]) * rs.uniform(1, 100)
        mk = ma[0] if rs.rand() < 0.5 else None
        cap = float(rs.choice([400.0, 50.0, 1e9]))
        coef, icpt = np.float32(rs.uniform(0.1, 50)), np.float32(rs.uniform(-1, 1) * (rs.rand() < 0.5))
        # matcher unprojection (src/matching/matcher.py:70-91)
        dm = np.abs(num[0]) + 0.5
        dm[rs.rand(H, W) < 0.2] = -1
        N = int(rs.choice([1, 17, 300]))
        uv = np.stack([rs.uniform(0, W - 1e-3, N), rs.uniform(0, H - 1e-3, N)], 1)
        Rm, Tm = (rand_rot(rs), rs.randn(3)) if rs.rand() < 0.6 else (None, None)
        flip = float(rs.choice([512.0, 100.0])) if rs.rand() < 0.7 else None
        fx, fy, cx, cy = rs.uniform(100, 900), rs.uniform(100, 900), rs.uniform(0, W), rs.uniform(0, H)
        c["depth_stats"] = dict(num=num, den=den, ma=ma, mb=mb, rel=rel, met=met, mk=mk, cap=cap, coef=coef, icpt=icpt,
                                dm=dm, uv=uv, Rm=Rm, Tm=Tm, flip=flip, cam=(fx, fy, cx, cy))
    return c


def expected(c):
    """What the reference computes for a case, in run_gpu's layout."""
    from oracle import la3d_oracle as O

    depth, K, R, t = c["depth"], c["K"], c["R"], c["t"]
    w = dict(unproject=[O.depth_to_points(depth[0][None], K[0], R, t),
                        np.stack([O.depth_to_points(d[None], K[0], R, t) for d in depth]),
                        np.stack([O.depth_to_points(d[None], k, R, t) for d, k in zip(depth, K)])],
             unproject_f32=O.depth_to_points(depth[0][None], K[0], R, t))
    if c["rle"] is not None:
        r = c["rle"]
        stats = np.array([O.mask_stats(m, r["bt"]) for m in r["masks"]])
        w.update(rle_decode=r["masks"], mask_stats=stats, mask_stats_rle=stats,
                 keep=[np.array([O.keep_instance(s, c["H"], from_rle, thr) for s in stats]) for from_rle, thr in zip((True, False), r["keep_thr"])])
    if c["poly"] is not None:
        pm = c["poly"]["masks"]
        w.update(poly_decode=pm, mask_stats_poly=np.array([O.mask_stats(m, c["rle"]["bt"]) for m in pm]))
    rec, Kb, ii = c["rec"], c["Kb"], c["ii"]
    with np.errstate(invalid="ignore", divide="ignore"):
        proj = O.project_boxes(rec, Kb if ii is None else Kb[ii], c["size"])
    proj[project_nan_rows(c)] = np.nan
    w.update(project_boxes=proj, iou=O.iou2d_matrix(c["b0"], c["b1"]))
    ds = c["depth_stats"]
    if ds is not None:
        num, den, ma, mb = ds["num"], ds["den"], ds["ma"], ds["mb"]
        med, cnt = [], []
        for i in range(len(num)):
            ov = ma[i] if mb is None else ma[i] & mb[i]
            with np.errstate(all="ignore"):
                med.append(np.float32(np.median(num[i][ov] / den[i][ov]) if ov.any() else np.float32(np.nan)))
            cnt.append(int(ov.sum()))
        rel, met, mk, cap = ds["rel"], ds["met"], ds["mk"], ds["cap"]
        with np.errstate(all="ignore"):
            valid = (~np.isinf(rel)) & (met < cap) & (True if mk is None else mk)
        sel_b = []
        for i in range(len(num)):
            with np.errstate(all="ignore"):
                v = (~np.isinf(num[i])) & (np.abs(den[i]) * 3 < cap) & (True if mk is None else ma[i])
            sel_b.append((num[i][v], (np.abs(den[i]) * 3)[v].astype(np.float32)))
        app = np.full_like(rel, 10000.0)
        sel = mk if mk is not None else ~np.isinf(rel)
        with np.errstate(all="ignore"):
            app[sel] = rel[sel] * ds["coef"] + ds["icpt"]
        dm, uv, (fx, fy, cx, cy), flip, Rm, Tm = ds["dm"], ds["uv"], ds["cam"], ds["flip"], ds["Rm"], ds["Tm"]
        d_of = dm[uv[:, 1].astype(int), uv[:, 0].astype(int)]
        okm = d_of != -1
        u = (flip - uv[:, 0]) if flip is not None else uv[:, 0]
        v = (flip - uv[:, 1]) if flip is not None else uv[:, 1]
        p3 = np.stack(((u - cx) * d_of / fx, (v - cy) * d_of / fy, d_of), -1).astype(np.float64)
        if Rm is not None:
            with np.errstate(invalid="ignore"):
                p3 = np.matmul(Rm, (p3.T - Tm.reshape(3, 1))).T
        p3[~okm] = np.nan
        w.update(median=(np.array(med, np.float32), np.array(cnt)), align_select=(rel[valid], met[valid]), align_select_batch=sel_b,
                 align_apply=app, matches=(p3, okm))
    return w


def project_nan_rows(c):
    """include/la3d.h: a box with a corner whose projection is NaN (a rejected box's NaN record, 0 / 0) gives 8 NaNs - Python's
    min() / max() over a NaN depend on its position in the list, which the oracle restates; those rows are held to "all NaN"."""
    rec, Kb, ii, Bb = c["rec"], c["Kb"], c["ii"], len(c["rec"])
    Kr = np.broadcast_to(Kb if ii is None else Kb[ii], (Bb, 3, 3)) if np.ndim(Kb) == 3 else np.broadcast_to(Kb, (Bb, 3, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        hp = np.einsum("bij,bvj->bvi", Kr, rec[:, 15:].reshape(Bb, 8, 3))
        return np.isnan(hp[..., :2] / hp[..., 2:3]).any((1, 2))


def run_gpu(c):
    """What the library computes for a case, as NumPy arrays.  Raises what a call raises."""
    import torch

    import labelany3d_amd as la
    from labelany3d_amd import consumers as C
    from labelany3d_amd import depth_align as DA
    from labelany3d_amd import masks as M
    from oracle import la3d_oracle as O

    np_ = lambda t: t.detach().cpu().numpy()   # noqa: E731
    depth, K, R, t = c["depth"], c["K"], c["R"], c["t"]
    g = dict(unproject=[np_(la.unproject(depth[0], K[0], R, t)), np_(la.unproject(depth, K[0], R, t)), np_(la.unproject(depth, K, R, t))],
             unproject_f32=np_(la.unproject(depth[0], K[0], R, t, out_dtype=torch.float32)))
    if c["rle"] is not None:
        r = c["rle"]
        stats = np_(M.mask_stats(r["masks"].astype(np.uint8) * r["u8_value"], r["bt"]))
        g.update(rle_decode=np_(M.rle_decode(r["rles"])), mask_stats=stats, mask_stats_rle=np_(M.mask_stats_rle(r["rles"], r["bt"])))
        # (the filter decisions from the reference's statistics: the filter is checked on its own)
        ref_stats = np.array([O.mask_stats(m, r["bt"]) for m in r["masks"]])
        g["keep"] = [np_(M.keep_instances(torch.as_tensor(ref_stats, dtype=torch.int32), c["H"], from_rle, thr))
                     for from_rle, thr in zip((True, False), r["keep_thr"])]
    if c["poly"] is not None:
        polys = M.pack_polygons(c["poly"]["segs"], c["H"], c["W"])
        g.update(poly_decode=np_(M.poly_decode(polys)), mask_stats_poly=np_(M.mask_stats_poly(polys, c["rle"]["bt"])))
    g.update(project_boxes=np_(C.project_boxes(c["rec"], c["Kb"], c["size"], image_index=c["ii"])), iou=np_(C.iou2d_matrix(c["b0"], c["b1"])))
    ds = c["depth_stats"]
    if ds is not None:
        med, cnt = (np_(x) for x in la.masked_ratio_median(ds["num"], ds["den"], ds["ma"], ds["mb"]))
        mk = ds["mk"]
        r_, m_ = DA.align_select(ds["rel"], ds["met"], mk, ds["cap"])
        rb, mbt, cb = DA.align_select_batch(ds["num"], np.abs(ds["den"]) * 3, ds["ma"] if mk is not None else None, ds["cap"])
        rb, mbt, cb = np_(rb), np_(mbt), np_(cb)
        pts, vld = C.unproject_matches(ds["dm"], ds["uv"], *ds["cam"], ds["flip"], ds["Rm"], ds["Tm"])
        g.update(median=(med, cnt), align_select=(np_(r_), np_(m_)),
                 align_select_batch=[(rb[i, :int(cb[i])], mbt[i, :int(cb[i])]) for i in range(len(cb))],
                 align_apply=np_(DA.align_apply(ds["rel"], ds["coef"], ds["icpt"], mk)), matches=(np_(pts), np_(vld)))
    return g


def check(c, want, got, counts=None):
    """Compare run_gpu's output with expected()'s.  Returns the failures as strings; counts (dict over COUNTS) tallies the checks."""
    n = dict.fromkeys(COUNTS, 0) if counts is None else counts
    fails = []
    # ---- unproject ----
    for mode in range(3):
        g, ref = got["unproject"][mode], want["unproject"][mode]
        ref = ref.reshape(g.shape)
        fin = np.isfinite(ref)
        if not np.array_equal(np.isnan(g), np.isnan(ref)) or not np.array_equal(np.isposinf(g), np.isposinf(ref)) or not np.array_equal(np.isneginf(g), np.isneginf(ref)):
            fails.append(f"unproject mode {mode}: NaN / inf pattern differs")
        elif fin.any():
            sc = max(1.0, float(np.abs(ref[fin]).max()))
            err = float(np.abs(g[fin] - ref[fin]).max())
            # (per point: |p| * a few ulp; the planes hold depths up to 1e3 next to 1e-2)
            if err > 1e-12 * sc:
                fails.append(f"unproject mode {mode}: {err:.3g} off (scale {sc:.3g})")
        n["unproject"] += 1
    g32 = got["unproject_f32"]
    r32 = want["unproject_f32"].reshape(g32.shape)
    fin = np.isfinite(r32) & (np.abs(r32) < 1e30)
    if fin.any():
        # (a float32 store of the float64 result: half an ulp = 6e-8 relative)
        bad = float((np.abs(g32[fin] - r32[fin]) / np.maximum(np.abs(r32[fin]), 1e-30)).max())
        if bad > 2e-7:
            fails.append(f"unproject f32: relative {bad:.3g}")
    # ---- run lengths / mask statistics / filters ----
    if c["rle"] is not None:
        r = c["rle"]
        B = len(r["masks"])
        if not np.array_equal(got["rle_decode"], want["rle_decode"]):
            fails.append(f"rle_decode differs at {int((got['rle_decode'] != want['rle_decode']).sum())} pixels")
        n["rle"] += B
        for name in ("mask_stats", "mask_stats_rle"):
            g, ref = got[name], want[name]
            if not np.array_equal(g, ref):
                bad = np.flatnonzero((g != ref).any(1))
                fails.append(f"{name} (boundary {r['bt']}) differs at {bad[:4].tolist()}: got {g[bad[:2]].tolist()} expected {ref[bad[:2]].tolist()}")
            n["stats"] += B
        for k, from_rle in enumerate((True, False)):
            if not np.array_equal(got["keep"][k], want["keep"][k]):
                fails.append(f"keep_instances(from_rle={from_rle}) differs")
            n["keep"] += B
    # ---- polygons ----
    if c["poly"] is not None:
        if not np.array_equal(got["poly_decode"], want["poly_decode"]):
            fails.append(f"poly_decode differs at {int((got['poly_decode'] != want['poly_decode']).sum())} pixels")
        if not np.array_equal(got["mask_stats_poly"], want["mask_stats_poly"]):
            fails.append(f"mask_stats_poly differs: got {got['mask_stats_poly'][:2].tolist()} expected {want['mask_stats_poly'][:2].tolist()}")
        n["poly"] += len(c["poly"]["segs"])
    # ---- consumers ----
    nan_row = project_nan_rows(c)
    g = got["project_boxes"]
    if not np.isnan(g[nan_row]).all():
        fails.append("project_boxes: a box with a NaN projection is not reported as 8 NaNs")
    g, ref = g[~nan_row], want["project_boxes"][~nan_row]
    fin = np.isfinite(ref) & np.isfinite(g)
    if not np.array_equal(np.isnan(g), np.isnan(ref)):
        fails.append("project_boxes: NaN pattern differs")
    elif not np.array_equal(np.isinf(g), np.isinf(ref)):
        fails.append("project_boxes: inf pattern differs")
    elif fin.any() and float((np.abs(g[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1.0)).max()) > 1e-12:
        fails.append(f"project_boxes: {float((np.abs(g[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1.0)).max()):.3g}")
    n["project"] += len(c["rec"])
    g, w = got["iou"], want["iou"]
    if not np.array_equal(np.isnan(g), np.isnan(w)):
        fails.append("iou2d_matrix: NaN pattern differs")
    elif (~np.isnan(w)).any() and float(np.abs(g - w)[~np.isnan(w)].max()) > 1e-12:
        fails.append(f"iou2d_matrix: {float(np.abs(g - w)[~np.isnan(w)].max()):.3g}")
    n["iou"] += want["iou"].size
    # ---- depth statistics, matcher ----
    ds = c["depth_stats"]
    if ds is not None:
        (med, cnt), (wmed, wcnt) = got["median"], want["median"]
        for i in range(len(wcnt)):
            if cnt[i] != wcnt[i]:
                fails.append(f"ratio median: count {cnt[i]} expected {wcnt[i]}"); continue
            if not (wmed[i] == med[i] or (np.isnan(wmed[i]) and np.isnan(med[i]))):
                fails.append(f"ratio median: got {med[i]!r} expected {wmed[i]!r} (count {cnt[i]})")
            n["median"] += 1
        (r_, m_), (wr, wm) = got["align_select"], want["align_select"]
        if not (np.array_equal(r_, wr, equal_nan=True) and np.array_equal(m_, wm, equal_nan=True)):
            fails.append("align_select differs")
        for i, ((rb, mbt), (wrb, wmbt)) in enumerate(zip(got["align_select_batch"], want["align_select_batch"])):
            if len(rb) != len(wrb) or not np.array_equal(rb, wrb, equal_nan=True) or not np.array_equal(mbt, wmbt, equal_nan=True):
                fails.append(f"align_select_batch differs at frame {i}")
        g, w = got["align_apply"], want["align_apply"]
        if not np.array_equal(g, w, equal_nan=True):
            fails.append(f"align_apply differs at {int((~((g == w) | (np.isnan(g) & np.isnan(w)))).sum())} pixels")
        n["align"] += 2 + len(ds["num"])
        (pts, vld), (p3, okm) = got["matches"], want["matches"]
        with np.errstate(invalid="ignore"):
            err = float(np.abs(pts[okm] - p3[okm]).max()) if okm.any() else 0.0
        if not np.array_equal(vld, okm) or not np.isnan(pts[~okm]).all():
            fails.append("unproject_matches: validity differs")
        elif okm.any() and err > 1e-12 * max(1.0, float(np.abs(p3[okm]).max())):
            fails.append(f"unproject_matches: {err:.3g}")
        n["matches"] += len(okm)
    return fails
