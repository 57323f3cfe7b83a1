"""The ground plane from depth (include/la3d.h "ground plane: RANSAC plane fit") restated in plain NumPy, and the generators of the
cases the CPU and GPU tests share.  Every product and sum of a trial's decisions is written out one by one, in the header's order - no
``np.cross``, no ``@``, nothing that may fuse a multiply with an add -, so the decisions can be held EXACTLY against the kernels'; the
refit is the exception and uses ``np.linalg.eigh``."""
import numpy as np

SEG = 1024                       # LA3D_PLANE_SEGMENT: samples one workgroup of the candidates pass judges
MAX_TRIALS = 1024                # LA3D_PLANE_MAX_TRIALS
OK, TOO_FEW, FAILED, BROKEN = 0, 1, 2, 3
FILL = np.float32(10000.0)       # what the depth alignment writes where it has no depth


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def select_ref(depth, candidates=None, step=4, near=0.0, far=np.inf):
    """pixel indices v * W + u of the kept grid pixels of one (H,W) float32 frame, raster order; ``candidates`` (H,W) bool or None"""
    d = np.asarray(depth, np.float32)
    H, W = d.shape
    out = []
    for v in range(0, H, step):
        for u in range(0, W, step):
            x = d[v, u]
            if np.isfinite(x) and x > 0 and np.float32(near) <= x <= np.float32(far) and (candidates is None or candidates[v, u]):
                out.append(v * W + u)
    return np.asarray(out, np.int32)


def _tol(pts, thr_abs, thr_rel):
    fin = np.isfinite(pts).all(axis=1)
    with np.errstate(all="ignore"):
        rel = thr_rel * pts[:, 2]
        return fin, thr_abs + rel


def trial_ref(pts, idx, thr_abs, thr_rel, cos2_tilt):
    """one trial on the (count,3) samples: None when it is skipped, else (inlier flags, a, w, s)"""
    n = len(pts)
    i, j, k = (int(t) for t in idx)
    if not (0 <= i < n and 0 <= j < n and 0 <= k < n):
        return None
    with np.errstate(all="ignore"):
        a, b, c = pts[i], pts[j], pts[k]
        ux, uy, uz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
        vx, vy, vz = c[0] - a[0], c[1] - a[1], c[2] - a[2]
        wx = uy * vz - uz * vy
        wy = uz * vx - ux * vz
        wz = ux * vy - uy * vx
        s = (wx * wx + wy * wy) + wz * wz
        if not (s > 0) or not np.isfinite(s) or not (wy * wy >= cos2_tilt * s):
            return None
        fin, tol = _tol(pts, thr_abs, thr_rel)
        dx, dy, dz = pts[:, 0] - a[0], pts[:, 1] - a[1], pts[:, 2] - a[2]
        e = (wx * dx + wy * dy) + wz * dz
        inl = fin & (e * e <= (tol * tol) * s)
    return inl, a, np.array([wx, wy, wz]), s


def refit_ref(pts, inl):
    """(plane (4,), eigen-gap (l1 - l0) / l2) of the eigh refit over the flagged samples, oriented so that n_y <= 0"""
    x = pts[inl]
    mu = x.mean(axis=0)
    c = x - mu
    lam, vec = np.linalg.eigh(c.T.dot(c))
    n = vec[:, 0] / np.linalg.norm(vec[:, 0])
    if n[1] > 0:
        n = -n
    return np.array([n[0], n[1], n[2], -float(n.dot(mu))]), float((lam[1] - lam[0]) / lam[2]) if lam[2] > 0 else 0.0


def recount_ref(pts, plane, thr_abs, thr_rel):
    """(flags, rms) of the final inliers under the given (reported) numbers: r = n_x x + n_y y + n_z z + d, |r| <= tol"""
    fin, tol = _tol(pts, thr_abs, thr_rel)
    with np.errstate(all="ignore"):
        r = ((plane[0] * pts[:, 0] + plane[1] * pts[:, 1]) + plane[2] * pts[:, 2]) + plane[3]
        inl = fin & (np.abs(r) <= tol)
    return inl, (float(np.sqrt(np.mean(r[inl] * r[inl]))) if inl.any() else float("nan"))


def ransac_ref(points, count, subsets, thr_abs, thr_rel=0.0, cos2_tilt=0.0, min_inliers=3):
    """one frame: ``points`` (n,3) float64 of which the first ``count`` are samples, ``subsets`` (T,3).  Returns a dict: status,
    best_trial, k_trial, and - fitted - trial_inliers (n,) bool, plane (eigh refit), gap"""
    n = len(points)
    out = dict(status=OK, best_trial=-1, k_trial=0, trial_inliers=np.zeros(n, bool), plane=np.full(4, np.nan), gap=float("nan"))
    if count < 0 or count > n:
        return dict(out, status=BROKEN)
    if count < 3:
        return dict(out, status=TOO_FEW)
    pts = np.asarray(points[:count], np.float64)
    best, k_best, flags = -1, -1, None
    for t, idx in enumerate(np.asarray(subsets)):
        r = trial_ref(pts, idx, thr_abs, thr_rel, cos2_tilt)
        if r is not None and int(r[0].sum()) > k_best:          # (strictly more: ties go to the lower t)
            best, k_best, flags = t, int(r[0].sum()), r[0]
    if best < 0 or k_best < min_inliers:
        return dict(out, status=FAILED)
    plane, gap = refit_ref(pts, flags)
    out["trial_inliers"][:count] = flags
    return dict(out, best_trial=best, k_trial=k_best, plane=plane, gap=gap)


def angle(a, b):
    """angle between two unit vectors, accurate for small angles"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(2.0 * np.arcsin(min(1.0, 0.5 * np.linalg.norm(a / np.linalg.norm(a) - b / np.linalg.norm(b)))))


# ---- the generators -------------------------------------------------------------------------------------------------------------
# A case is a dict: name, points (n,3) float64, count, subsets (T,3) int32.  A call has ONE set of scalars for all its frames, so the cases
# share theirs: a sample at depth z is an inlier within THR_ABS + THR_REL * z, and MAX_TILT keeps walls out.
THR_ABS, THR_REL, MAX_TILT = 0.01, 0.001, 0.6
NORMAL = np.array([0.06, -0.93, -0.36]) / np.linalg.norm([0.06, -0.93, -0.36])     # a floor under a pitched, slightly rolled camera
HEIGHT = 1.4


def _floor(rng, m, noise=0.001):
    """m points of the plane NORMAL . x + HEIGHT = 0 in front of the camera, 2 .. 9 m away, with `noise` metres across it"""
    e1 = np.cross(NORMAL, [0.0, 0.0, 1.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(NORMAL, e1)
    s, t = rng.uniform(-2.5, 2.5, m), rng.uniform(2.0, 9.0, m)
    return -HEIGHT * NORMAL + s[:, None] * e1 + t[:, None] * e2 * np.sign(e2[2]) + rng.normal(0.0, noise, m)[:, None] * NORMAL


def _draw(rng, count, T):
    """T triples of distinct indices into [0, count)"""
    if count < 3:
        return np.zeros((T, 3), np.int32)
    return np.stack([rng.choice(count, 3, replace=False) for _ in range(T)]).astype(np.int32)


def _case(name, points, count, subsets):
    return dict(name=name, points=np.ascontiguousarray(points, np.float64), count=int(count), subsets=np.ascontiguousarray(subsets, np.int32))


def clean(n, T, seed=0):
    rng = np.random.default_rng(1000 + seed)
    return _case("clean", _floor(rng, n), n, _draw(rng, n, T))


def wall(n, T, seed=0):
    """a floor, 40 % outliers among floor + outliers, and a LARGER wall: without max_tilt the wall wins, with it the floor"""
    rng = np.random.default_rng(2000 + seed)
    nw = (n * 9) // 20
    no = ((n - nw) * 2) // 5
    nf = n - nw - no
    wl = np.stack([rng.uniform(-3, 3, nw), rng.uniform(-2.0, 1.2, nw), 6.0 + rng.normal(0.0, 0.001, nw)], axis=1)
    out = np.stack([rng.uniform(-3, 3, no), rng.uniform(-2.0, 1.3, no), rng.uniform(1.5, 9.0, no)], axis=1)
    pts = np.concatenate([_floor(rng, nf), wl, out])
    pts = pts[rng.permutation(n)]
    return _case("wall", pts, n, _draw(rng, n, T))


def collinear(n, T, seed=0):
    """every sample on one line, coordinates small integers: every cross product is exactly zero, every trial skipped"""
    rng = np.random.default_rng(3000 + seed)
    t = rng.integers(-500, 500, n).astype(np.float64)
    return _case("collinear", np.stack([t, 2.0 * t + 1.0, 3.0 * t - 2.0], axis=1), n, _draw(rng, n, T))


def repeated(n, T, seed=0):
    """every second trial repeats an index - among them what would be the first trial"""
    c = clean(n, T, 10 + seed)
    sub = c["subsets"].copy()
    sub[0::2, 1] = sub[0::2, 0]
    if T > 2:
        sub[3, 2] = sub[3, 1]
    return dict(c, name="repeated", subsets=sub)


def out_of_range(n, T, seed=0):
    """indices at count, beyond the row, negative; the row is longer than the count"""
    c = clean(n, T, 20 + seed)
    count = max(n - 7, min(n, 3))
    sub = _draw(np.random.default_rng(2500 + seed), count, T)
    bad = (count, n, n + 5, -1, -2147483648, 2147483647)
    for t in range(0, T, 3):
        sub[t, t % 3] = bad[(t // 3) % len(bad)]
    return dict(c, name="out_of_range", count=count, subsets=sub)


def non_finite(n, T, seed=0):
    """NaN and infinities among the points, handed in directly; some trials draw them"""
    c = clean(n, T, 30 + seed)
    pts = c["points"].copy()
    rng = np.random.default_rng(3500 + seed)
    hit = rng.choice(n, max(1, n // 5), replace=False)
    vals = (np.nan, np.inf, -np.inf)
    for q, i in enumerate(hit):
        pts[i, q % 3] = vals[(q // 3) % 3]
    sub = c["subsets"].copy()
    sub[1::4, 0] = hit[np.arange(len(sub[1::4])) % len(hit)]
    return dict(c, name="non_finite", points=pts, subsets=sub)


def broken(n, T, seed=0):
    c = clean(n, T, 50 + seed)
    return dict(c, name="broken", count=(n + 1 if seed % 2 == 0 else -1))


def ties(n, T, seed=0):
    """the same triple at several trials: equal k, the lowest t must win; noisy floor so that trials differ in k"""
    rng = np.random.default_rng(6000 + seed)
    pts = _floor(rng, n, noise=0.008)
    sub = _draw(rng, n, T)
    c = _case("ties", pts, n, sub)
    if T >= 4:
        ks = [(-1 if r is None else int(r[0].sum())) for r in (trial_ref(pts, s, THR_ABS, THR_REL, cos2(MAX_TILT)) for s in sub)]
        b = int(np.argmax(ks))
        for t in (T - 1, T // 2, min(b + 1, T - 1)):
            sub[t] = sub[b]
        if b > 0:
            sub[[0, b]] = sub[[b, 0]]            # (and once with the tie's first member at t = 0)
            sub[T - 1] = sub[0]
    return dict(c, subsets=sub)


def tiny(n, T, seed=0):
    """n = 0, 2, 3, 4: a well-shaped triangle (and a fourth point on its plane) - or too few samples"""
    base = np.array([[-1.0, 1.2, 3.0], [1.5, 1.1, 3.5], [0.2, 0.6, 6.0], [0.5, 0.9, 4.5]])
    base[3] = base[0] + 0.3 * (base[1] - base[0]) + 0.4 * (base[2] - base[0])
    rng = np.random.default_rng(7000 + seed)
    sub = _draw(rng, n, T) if n >= 3 else np.zeros((T, 3), np.int32)
    return _case("tiny", base[:n], n, sub)


GENERATORS = (clean, wall, collinear, repeated, out_of_range, non_finite, broken, ties)
SAMPLE_COUNTS = (0, 2, 3, 4, SEG - 1, SEG, SEG + 1)
TRIAL_COUNTS = (1, 64, 65, MAX_TRIALS)
BATCHES = (1, 3, 65)


def batch_cases(P, n, T, seed=0):
    """P cases of capacity n and T trials, cycling through the generators (n < 5: the tiny cases)"""
    if n < 5:
        return [tiny(n, T, seed + p) for p in range(P)]
    return [GENERATORS[(p + seed) % len(GENERATORS)](n, T, seed + p) for p in range(P)]


def all_batches():
    """(tag, cases) of every batch the GPU tests run: every sample count, every trial count, every batch size, every generator"""
    out = []
    for n in SAMPLE_COUNTS:
        out.append((f"n{n}", batch_cases(3, n, 64, seed=n)))
    for T in TRIAL_COUNTS:
        out.append((f"T{T}", batch_cases(1 if T == MAX_TRIALS else 3, SEG + 1, T, seed=T)))
    for P in BATCHES:
        out.append((f"P{P}", batch_cases(P, 300, 64, seed=P)))
    out.append(("generators", [g(SEG + 1, 65, 7) for g in GENERATORS]))
    return out


def stack(cases):
    """cases of one T -> (points (P,n,3) with NaN behind every case's own row, counts (P,), subsets (P,T,3))"""
    P, n = len(cases), max(max(len(c["points"]) for c in cases), 1)
    pts = np.full((P, n, 3), np.nan)
    for p, c in enumerate(cases):
        pts[p, :len(c["points"])] = c["points"]
    return pts, np.array([c["count"] for c in cases], np.int64), np.stack([c["subsets"] for c in cases])


def cos2(max_tilt):
    return 0.0 if max_tilt is None else float(np.cos(np.float64(max_tilt)) ** 2)


def expected(c, n=None, min_inliers=3, max_tilt=MAX_TILT):
    """ransac_ref of a case (on a row of capacity n >= len(points)) under the shared scalars; ``min_inliers`` above the best k is the
    case "no plane worth the name" (status 2)"""
    pts = c["points"]
    if n is not None and n > len(pts):
        pts = np.concatenate([pts, np.full((n - len(pts), 3), np.nan)])
    return ransac_ref(pts, c["count"], c["subsets"], THR_ABS, THR_REL, cos2(max_tilt), min_inliers)


# ---- the scene the feature exists for -------------------------------------------------------------------------------------------
def scene(H=96, W=128, f=120.0, height=1.4, pitch=0.35, roll=0.07, box=(1.0, 0.7, 1.0), box_at=(0.15, 3.1), box_yaw=0.5, sky_rows=8):
    """A camera `height` metres over a plane, pitched down and rolled, one box (width, depth, HEIGHT) standing on the plane, rendered
    analytically: depth (H,W) float32 with a band of 10000.0 fill at the top, the box's instance mask, K, the true plane (n, d) in
    camera coordinates (n_y < 0) and the box's height."""
    K = np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])
    up = np.array([np.sin(roll) * np.cos(pitch), -np.cos(roll) * np.cos(pitch), -np.sin(pitch)])      # the plane's normal, camera frame
    fwd = np.array([0.0, 0.0, 1.0]) - up * up[2]
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up)                                                                       # (right, up, fwd): the world's axes
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.stack([(u - K[0, 2]) / f, (v - K[1, 2]) / f, np.ones_like(u)], axis=-1)               # z = 1: the ray parameter is the depth
    world = np.stack([rays.dot(right), rays.dot(up), rays.dot(fwd)], axis=-1)                        # ray directions in world axes, origin (0, height, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ground = np.where(world[..., 1] < 0, -height / world[..., 1], np.inf)
        # the box in world axes: centre (x, bh / 2, z) relative to the point under the camera, turned by box_yaw about up
        bw, bd, bh = box
        c, s = np.cos(box_yaw), np.sin(box_yaw)
        org = np.array([0.0, height, 0.0]) - np.array([box_at[0], bh / 2.0, box_at[1]])
        rot = np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])
        o, d = rot.dot(org), world.dot(rot.T)
        half = np.array([bw / 2.0, bh / 2.0, bd / 2.0])
        t1, t2 = (-half - o) / d, (half - o) / d
        tn, tf = np.minimum(t1, t2).max(axis=-1), np.maximum(t1, t2).min(axis=-1)
    hit = (tn <= tf) & (tn > 0)
    mask = hit & (tn < t_ground)
    depth = np.where(mask, tn, t_ground)
    depth[~np.isfinite(depth) | (depth > 60.0)] = FILL
    depth[:sky_rows] = FILL
    mask[:sky_rows] = False
    return dict(depth=depth.astype(np.float32), mask=mask, K=K, normal=up, d=height, box_height=bh)
