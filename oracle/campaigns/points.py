"""The randomised differential campaign of the point-cloud entry (la3d_fit_points through labelany3d_amd.fit_points: estimate_bbox for
explicit clouds - what the reference's harness calls per mesh): case generator, oracle, GPU runs and the checkers.
profiles/r06/fuzz_points.py drives it at scale; tests/test_gpu_differential.py runs a committed slice of its seeds.

One CASE = one launch over B clouds of 0 ... 5000 rows (sizes around the kernel's and the reference's thresholds: 1, 2, 19 / 20 - the
two PCA solvers of scikit-learn -, 500 / 501 - the reference's subsample -, 512 / 513 and 2048 / 2049 - the hull kernel's two
forms), shaped as blobs, boxes, slivers, planes and lattices with jitter, at the origin or tens of metres away from it, with NaN
rows (which the reference drops) and infinite rows (which it rejects), ground planes for all / some / none of the clouds, in
full-cloud and in reference-subsample mode, with the yaw from PCA and from the convex hull; every case through the default launch,
with the one-wave-per-cloud hint forced on and off and (hull) with the 512-row form forced off, and - full-cloud cases - the first
clouds through the scalar drop-in.  EVERY record is compared with the CPU oracle (oracle/la3d_oracle.py) under
tests/test_gpu_parity.py::assert_records' rule; hull records additionally by their own footprint area when the oracle's minimum is
tied within rounding (two hull edges whose rectangles differ by less than 1e-12).
The oracle is test infrastructure: it is the checker here."""
import numpy as np

SIZES = [0, 1, 2, 3, 5, 8, 19, 20, 21, 64, 100, 300, 499, 500, 501, 512, 513, 700, 1500, 2047, 2048, 2049, 5000]


def one_cloud(rs, n):
    kind = rs.randint(0, 6)
    off = np.array([rs.uniform(-30, 30), rs.uniform(-2, 2), rs.uniform(0, 60)]) * (rs.rand() < 0.7)
    yaw = rs.uniform(-np.pi, np.pi)
    R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    if kind == 0:
        p = rs.randn(n, 3) * rs.uniform(0.05, 3, 3)
    elif kind == 1:
        p = rs.uniform(-1, 1, (n, 3)) * rs.uniform(0.1, 4, 3)
    elif kind == 2:                          # a sliver
        p = rs.randn(n, 3) * np.array([rs.uniform(0.5, 3), rs.uniform(0.1, 1), 10 ** rs.uniform(-5, -1)])
    elif kind == 3:                          # a vertical plane
        p = rs.uniform(-1, 1, (n, 3)) * np.array([rs.uniform(0.5, 3), rs.uniform(0.5, 3), 0.0])
    elif kind == 4:                          # a jittered lattice (many hull points on every side)
        k = max(1, int(np.ceil(np.sqrt(n))))
        g = np.stack(np.meshgrid(np.arange(k), np.arange(k)), -1).reshape(-1, 2)[:n].astype(float)
        p = np.stack([g[:, 0] * 0.1, rs.uniform(0, 1, len(g)), g[:, 1] * 0.07], 1) + 1e-3 * rs.randn(len(g), 3)
    else:                                    # points on a circle (every point a hull vertex)
        t = rs.uniform(0, 2 * np.pi, n)
        p = np.stack([2 * np.cos(t), rs.uniform(0, 1, n), 1.3 * np.sin(t)], 1) * rs.uniform(0.2, 3)
    p = p @ R.T + off
    if n and rs.rand() < 0.3:
        bad = rs.rand(n) < 10 ** rs.uniform(-3, -0.5)
        p[bad, rs.randint(0, 3, int(bad.sum()))] = np.nan
    if n and rs.rand() < 0.04:
        p[rs.randint(n), rs.randint(3)] = [np.inf, -np.inf][rs.randint(2)]
    return p


def make_case(seed):
    rs = np.random.RandomState(seed)
    B = int(rs.choice([1, 2, 5, 16, 33, 64]))
    big = rs.rand() < 0.5
    clouds = [one_cloud(rs, int(rs.choice(SIZES if big else SIZES[:14]))) for _ in range(B)]
    gk = rs.randint(0, 4)
    ground = None
    if gk >= 1:
        ground = np.array([[0.05, -0.97, 0.1, 1.2]] * B) + 0.05 * rs.randn(B, 4)
        if gk == 3:
            for n in range(B):
                r = rs.rand()
                if r < 0.25:
                    ground[n, 0] = np.nan
                elif r < 0.32:
                    ground[n] = [0, -1, 0, 1.0]
    sidx = None
    if rs.rand() < 0.4:
        sidx = np.zeros((B, 500), np.int32)
        for n, c in enumerate(clouds):
            if len(c) > 500:
                sidx[n] = rs.randint(0, len(c), 500)
    return dict(seed=seed, B=B, clouds=clouds, ground=ground, sidx=sidx)


def oracle_case(seed):
    from oracle import la3d_oracle as O

    c = make_case(seed)
    out = {}
    for method in ("pca", "convex_hull"):
        recs, sts, nvs, kaps, tied = [], [], [], [], []
        for n, pts in enumerate(c["clouds"]):
            g = None if c["ground"] is None or np.isnan(c["ground"][n, 0]) else c["ground"][n]
            ri = c["sidx"][n] if (c["sidx"] is not None and len(pts) > O.SUBSAMPLE) else False
            rec, st, aux = O.fit_points(pts, g, ri, method)
            recs.append(rec); sts.append(st); nvs.append(aux.get("n_valid", 0)); kaps.append(aux.get("kappa", np.nan))
        out[method] = (np.array(recs), np.array(sts, np.int32), np.array(nvs, np.int64), np.array(kaps))
    return seed, out


def footprint_area(rec):
    return rec[3] * rec[5]   # dims = [dz, dy, dx]


RUNS = [dict(), dict(small_clouds=True), dict(small_clouds=False), dict(hull_512=False)]


METHODS = ("pca", "convex_hull")


def runs_for(method):
    return [r for r in RUNS if not ("hull_512" in r and method != "convex_hull")]


def new_tally():
    return dict(n_rec=0, n_tie=0, n_cap=0, n_hull_tied=0, n_hull_flat=0, n_scalar=0)


def run_gpu(c, method, r):
    """One launch of a case -> (boxes, status, aux) as NumPy arrays.  Raises what the call raises."""
    import labelany3d_amd as la

    b, stg, aux = la.fit_points(c["clouds"], ground=c["ground"], sample_idx=c["sidx"], method=method, **r)
    return b.detach().cpu().numpy(), stg.detach().cpu().numpy(), aux.detach().cpu().numpy()


def check_run(c, ref_m, method, r, got, tally=None):
    """Compare one launch (got = run_gpu's (boxes, status, aux)) with the oracle's ref_m = oracle_case(seed)[1][method] = (rec,
    status, n_valid, kappa).  Returns the failures as strings."""
    from tests.test_gpu_parity import assert_records, reference_axis_noise

    t = new_tally() if tally is None else tally
    rec, st, nv, kap = ref_m
    b, stg, aux = got
    # the hull kernel holds 2048 valid rows per cloud (512 in its small form, which the wrapper only takes when every cloud fits):
    # beyond that status 5 where the oracle fits
    capped = (stg == 5) & (st == 0) & (nv > 2048) if method == "convex_hull" else np.zeros(c["B"], bool)
    t["n_cap"] += int(capped.sum())
    same = (stg == st) | capped
    if not same.all():
        bad = np.flatnonzero(~same)
        return [f"status at {bad[:5].tolist()}: got {stg[bad][:5].tolist()} expected {st[bad][:5].tolist()} sizes {[len(c['clouds'][i]) for i in bad[:5]]}"]
    ok = (st == 0) & ~capped
    if not np.isnan(b[~ok]).all():
        return ["a rejected cloud's record is not NaN"]
    if not np.array_equal(aux[ok, 1], nv[ok]):
        return ["n_valid differs"]
    tie = ok & ~(aux[:, 3] >= 1e-9) if method == "pca" else np.zeros(c["B"], bool)
    t["n_tie"] += int(tie.sum())
    noise = reference_axis_noise(kap, aux[:, 1], aux[:, 3]) if method == "pca" else np.zeros(c["B"])
    tag = f"seed {c['seed']} B={c['B']} {method} ground={'no' if c['ground'] is None else 'yes'} sample={c['sidx'] is not None} {r}"
    fails = []
    for n in np.flatnonzero(ok & ~tie):
        try:
            assert_records(b[n:n + 1], rec[n:n + 1], tag, gap=aux[n:n + 1, 3] if method == "pca" else None, noise=noise[n:n + 1])
            t["n_rec"] += 1
        except AssertionError as e:
            # convex hull: two edges whose enclosing rectangles have the same area within rounding - either is the reference's
            # "first strict minimum" depending on the last bit (the oracle documents it: tests avoid exact ties)
            # (the height - the extent along the ground normal - does not depend on the yaw: it must agree either way)
            ext = max(np.abs(rec[n, 3:6]).max(), 1e-300)
            if method == "convex_hull" and abs(footprint_area(b[n]) - footprint_area(rec[n])) <= 1e-9 * max(footprint_area(rec[n]), 1e-300) \
                    and np.abs(b[n, 4] - rec[n, 4]) <= 1e-9 * max(ext, 1.0):
                t["n_hull_tied"] += 1
                continue
            # a footprint without area (collinear within rounding): whether a 2-D hull exists at all is decided by the last
            # bits - Qhull reports such input as flat and the reference falls back to PCA, or not, by its own tolerance
            if method == "convex_hull" and max(footprint_area(b[n]), footprint_area(rec[n])) <= 1e-9 * ext * ext \
                    and np.abs(b[n, 4] - rec[n, 4]) <= 1e-9 * max(ext, 1.0):
                t["n_hull_flat"] += 1
                continue
            what = [ln for ln in str(e).splitlines() if "center" in ln or "R_cam" in ln or "vertices" in ln]
            fails.append(f"cloud {n} ({len(c['clouds'][n])} rows, n_valid {int(aux[n, 1])}, gap {aux[n, 3]:.3g}, kappa {kap[n]:.3g}): "
                         f"{what[0].strip() if what else 'mismatch'} | d center/dims {np.abs(b[n, :6] - rec[n, :6]).max():.3g} "
                         f"dR {np.abs(b[n, 6:15] - rec[n, 6:15]).max():.3g} area {footprint_area(b[n]):.6g} vs {footprint_area(rec[n]):.6g}")
    return fails


SCALAR_CLOUDS = 6   # the scalar drop-in runs the first clouds of every full-cloud case


def scalar_clouds(c):
    return range(min(c["B"], SCALAR_CLOUDS)) if c["sidx"] is None else range(0)


def run_scalar(c, method, n, ref_st):
    """The scalar drop-in (la3d_estimate_bbox_host: the cloud pulled from pinned host memory into LDS by a kernel of its own) on cloud
    n, errors as the reference's exceptions -> (status, record, aux); status from the exception's message (statuses 1 and 2 share
    it: the oracle's ref_st decides between them)."""
    import contextlib
    import io

    from labelany3d_amd import util_3dbox as U

    g = None if c["ground"] is None or np.isnan(c["ground"][n, 0]) else c["ground"][n]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            r1, a1 = U._fit_one(c["clouds"][n], g, method, subsample=False)
        return 0, r1, a1
    except ValueError as e:
        got_st = [k for k, v in U._MESSAGES.items() if v == str(e)]
        return (int(ref_st) if int(ref_st) in got_st else (got_st[0] if got_st else -1)), None, None


def check_scalar(c, ref_m, method, n, got):
    """Compare one scalar drop-in call (got = run_scalar's (status, record, aux)) with the oracle.  Returns failures as strings."""
    from tests.test_gpu_parity import assert_records, reference_axis_noise

    rec, st, nv, kap = ref_m
    got_st, r1, a1 = got
    if got_st == 5 and st[n] == 0 and nv[n] > 2048 and method == "convex_hull":
        return []
    if got_st != st[n]:
        return [f"status {got_st} expected {int(st[n])}"]
    if got_st != 0 or (method == "pca" and not a1[3] >= 1e-9):
        return []
    try:
        assert_records(r1[None], rec[n:n + 1], f"seed {c['seed']} cloud {n} scalar drop-in {method}", gap=a1[3:4] if method == "pca" else None,
                       noise=reference_axis_noise(kap[n:n + 1], a1[1:2], a1[3:4]) if method == "pca" else None)
    except AssertionError as e:
        # (as in check_run: a tied minimum-area edge, or a footprint without area - the height agrees either way)
        ext = max(np.abs(rec[n, 3:6]).max(), 1e-300)
        if method == "convex_hull" and (abs(footprint_area(r1) - footprint_area(rec[n])) <= 1e-9 * max(footprint_area(rec[n]), 1e-300)
                                        or max(footprint_area(r1), footprint_area(rec[n])) <= 1e-9 * ext * ext) \
                and np.abs(r1[4] - rec[n, 4]) <= 1e-9 * max(ext, 1.0):
            return []
        return [str(e).strip().splitlines()[-1][:200]]
    return []
