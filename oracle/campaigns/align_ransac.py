"""The differential campaign of the batched RANSAC scale fit (include/la3d.h "depth alignment: RANSAC scale fit"; kernels:
labelany3d_amd/csrc/la3d_align.hip; Python: ransac_scale_batch / ransac_subsets / align_depth_batch).

The oracle is tests/align_ransac_cases.ransac_scale, the one NumPy text the header points to, imported - not restated.  Subsets are
drawn with plain NumPy (``rs.permutation(n)[:m]``), so the campaign needs no scikit-learn.

A case (make_case(seed)) is a batch of P frames in padded (P, n_cap) rows with their own counts, every frame drawn from a family and a
size of its own (FAMILIES of tests/align_ransac_cases.py, plus a frame with one non-finite sample, a frame without samples and a frame
whose count exceeds the row), one min_samples / max_trials / stop_probability for the call, explicit subsets (P, T, m_cap) with -1 or
in-range garbage behind m, in some cases an m_cap shorter than one frame's m; and, in most cases, a small stack of (Pd, H, W) depth
frames with masks, +-inf in the relative depth and a cap for the chain select -> fit -> apply.

Classes, from the oracle alone.  status, n_trials, n_inliers and best_trial are held exactly and coef to the adjacent float32 (both
sides round float64 quotients that differ by summation order only) on every DECIDED frame.  A frame is UNDECIDED where its outcome
hangs on float64 rounding, for one of three causes found in the oracle's own trace of the loop:

  score   two trials the loop compares have equal k, slopes that differ in their bits, and scores closer than the rounding bound of
          R^2 = 1 - num / den.  The bound, per trial, from the oracle's sums (eps = 2^-52, k inliers, c the frame's median):
            num  k non-negative squares added in any order: relative error <= (k + 2) eps.  The header fixes the inlier test's
                 residual as float32(y - float32(x a)) and the score as "R^2 in float64" without saying whether the squared
                 residual is that float32 or the float64 difference; both are computed here and their distance is part of d_num:
                 d_num = |num32 - num64| + (k + 2) eps max(num32, num64)
            den  the oracle adds (y - mean)^2; a kernel may add about any origin o and in any order, den = S_o - (sum (y - o))^2 / k,
                 where S_o = sum (y - o)^2 carries (k + 2) eps S_o and the subtracted square, which is <= S_o (Cauchy-Schwarz), as
                 much again; with the median as origin: d_den = 2 (k + 4) eps S_c
            R^2  |d score| <= e = d_num / den + num d_den / (den (den - d_den)) + 2 eps (1 + |score|); infinite where d_den >= den
          Two scores whose distance is at most 2 (e_t + e_best) may compare either way.  A zero-variance score (all inlier y equal)
          is exact on both sides: e = 0; a NaN score (k < 2) compares false on both sides.
  limit   the quotient log(nom) / log(denom) of the dynamic trial limit lies within 1e-9 relative of an integer <= max_trials: the
          ceil may give that integer or the next.  (Not where nom == denom bit for bit - a stop probability of 1 with every sample
          an inlier, both clamped to eps: equal arguments have equal logarithms and v / v is exactly 1 on both sides.)
  slope   a trial's float64 quotient sum xy / sum xx lies within 2^-40 relative of the boundary between two float32: either may be
          the trial's slope
Trials with bit-identical slopes have identical inlier sets and sums: both sides are deterministic there, the frame stays decided.
For an undecided frame the oracle's loop is walked again with the ambiguous step answered the other way (the ``alt`` argument of
ransac_scale), recursively; status is still exact, and (best_trial, n_inliers, n_trials, coef to the adjacent float32) must be those
of one of these walks.  At most 5 % of the frames may be undecided (tests/test_differential_checkers.py asserts it on the CPU).

Frames with thr == 0 (one sample, constant y, more than half of the y equal) are held to the restatement like every other frame and
counted on a tally line of their own: there the inlier test is an exact float32 equality and scikit-learn itself may raise where the
restatement fits (tests/align_ransac_cases.py).
"""
import numpy as np

from tests import align_ransac_cases as R

PS = [1, 2, 5, 17, 70]
SIZES = [1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 12289, 16385, 20000]
DRAW_ONLY = [16384, 65536, 65537]          # the draw-only leg: ransac_subsets without a fit
DRAW_ONLY_TRIALS = 5
MIN_SAMPLES = [0.05, 0.2, 0.5, 1, 2, "n"]  # "n": the size of one of the case's frames (smaller frames fail: m > n)
TRIALS = [1, 7, 64, 65, 100, 1024]
STOPS = [0.0, 0.5, 0.99, 1.0]
FRAMES_HW = [(1, 1), (2, 3), (7, 9), (48, 64), (61, 83)]
SPECIAL = ["non-finite sample", "count 0", "count exceeds the row"]
SEG = 4096                                 # samples per segment row (AR_SEG of la3d_align.hip)
FILL = np.float32(10000.0)
EPS = 2.0 ** -52
FIELDS = ("coef", "n_inliers", "n_trials", "best_trial", "status")
UNDECIDED_CAP = 0.05


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def _subsets(rs, ns, ms, T, m_cap, garbage):
    sub = np.full((len(ns), T, m_cap), -1, np.int32)
    for p, (n, m) in enumerate(zip(ns, ms)):
        if not 1 <= m <= min(n, m_cap):
            continue
        if garbage and m < m_cap:
            sub[p, :, m:] = rs.randint(0, n, (T, m_cap - m))
        for t in range(T):
            sub[p, t, :m] = rs.permutation(n)[:m]
    return sub


def _size_pool(P, T, p):
    if T == 1024:
        return [n for n in SIZES if n <= 1025]
    if P <= 5 or (P == 17 and p == 0):
        return SIZES
    if P == 17:
        return [n for n in SIZES if n <= 4097]
    return [n for n in SIZES if n <= (8193 if p == 0 else 1025)]


def _depth_part(rs):
    names = list(R.FAMILIES)
    Pd = int(rs.choice([1, 2, 3]))
    H, W = FRAMES_HW[rs.randint(len(FRAMES_HW))]
    rel, met, fam = np.empty((Pd, H, W), np.float32), np.empty((Pd, H, W), np.float32), []
    for p in range(Pd):
        fam.append(names[rs.randint(len(names))])
        x, y = R.FAMILIES[fam[-1]](rs, H * W)
        rel[p], met[p] = x.reshape(H, W), y.reshape(H, W)
        holes = rs.rand(H, W) < rs.choice([0.0, 0.1, 0.3])
        rel[p][holes] = rs.choice([np.inf, -np.inf], int(holes.sum()))
    mask = None
    if rs.rand() < 0.6:
        mask = rs.rand(Pd, H, W) < np.asarray(rs.choice([0.0, 0.4, 0.9, 1.0], Pd, p=[0.1, 0.3, 0.4, 0.2]))[:, None, None]
    cap = float(rs.choice([400.0, float(np.median(met[0])), 1e30]))
    if rs.rand() < 0.1:
        rel[rs.randint(Pd)].reshape(-1)[rs.randint(H * W)] = np.nan     # kept by ~isinf: a failed fit where it is selected
    valid = (~np.isinf(rel)) & (met < np.float32(cap))
    if mask is not None:
        valid &= mask
    ns = [int(v.sum()) for v in valid]
    min_samples = float(rs.choice([0.05, 0.2, 0.5]))
    T = int(rs.choice([7, 100]))
    ms = [R.subset_size(min_samples, n) for n in ns]
    sub = _subsets(rs, ns, ms, T, max(ms + [1]), False)
    return dict(P=Pd, H=H, W=W, rel=rel, met=met, mask=mask, cap=cap, fam=fam, valid=valid, ns=ns, min_samples=min_samples, T=T, sub=sub)


def make_case(seed):
    rs = np.random.RandomState(seed)
    names = list(R.FAMILIES)
    T = int(rs.choice(TRIALS, p=[0.08, 0.1, 0.1, 0.1, 0.5, 0.12]))
    P = int(rs.choice(PS, p=[0.2, 0.2, 0.3, 0.2, 0.1]))
    if T == 1024:
        P = min(P, 5)
    fam, data, ns = [], [], []
    for p in range(P):
        u = rs.rand()
        f = SPECIAL[int(u / 0.04)] if u < 0.12 else names[rs.randint(len(names))]
        pool = _size_pool(P, T, p)
        n = 0 if f == "count 0" else int(pool[rs.randint(len(pool))])
        if f in SPECIAL:
            x, y = R.FAMILIES["outliers 30 %"](rs, n)
            if f == "non-finite sample":
                (x if rs.randint(2) else y)[rs.randint(n)] = rs.choice([np.nan, np.inf, -np.inf])
        else:
            x, y = R.FAMILIES[f](rs, n)
        fam.append(f); data.append((x, y)); ns.append(n)
    n_cap = max(ns + [1]) + int(rs.choice([0, 0, 1, 3]))
    pad = np.float32(np.nan) if seed & 1 else np.float32(777.0)          # what lies behind a frame's count is never read
    xs, ys = np.full((P, n_cap), pad, np.float32), np.full((P, n_cap), pad, np.float32)
    counts = np.asarray(ns, np.int64)
    for p, (x, y) in enumerate(data):
        xs[p, :ns[p]], ys[p, :ns[p]] = x, y
        if fam[p] == "count exceeds the row":
            counts[p] = n_cap + 1 + rs.randint(3)
    kind = MIN_SAMPLES[rs.randint(len(MIN_SAMPLES))]
    min_samples = kind
    if kind == "n":
        own = [n for n, f in zip(ns, fam) if f not in SPECIAL and 1 <= n <= 4097]
        min_samples = float(own[rs.randint(len(own))]) if own else 2.0
    min_samples = float(min_samples)
    ms = [R.subset_size(min_samples, n) if f != "count exceeds the row" else 0 for n, f in zip(ns, fam)]
    fits = sorted({m for m, n in zip(ms, ns) if 1 <= m <= n})
    m_top = fits[-1] if fits else 1
    u = rs.rand()
    cap_kind = "short" if (u < 0.1 and len(fits) >= 2) else ("wide" if u < 0.55 else "tight")
    m_cap = fits[-2] if cap_kind == "short" else m_top + (int(rs.randint(1, 6)) if cap_kind == "wide" else 0)
    garbage = bool(rs.randint(2))
    sub = _subsets(rs, ns, ms, T, m_cap, garbage)
    stop = float(rs.choice(STOPS, p=[0.12, 0.13, 0.6, 0.15]))
    draw_seed = int(rs.randint(0, 2 ** 31))
    if rs.randint(2):
        draw_seed = (draw_seed << 33) | 1
    extra = [n for n in DRAW_ONLY if rs.rand() < 0.15]
    depth = _depth_part(rs) if rs.rand() < 0.6 else None
    return dict(seed=seed, P=P, T=T, n_cap=n_cap, fam=fam, ns=ns, x=xs, y=ys, counts=counts, kind=kind, min_samples=min_samples, ms=ms,
                m_cap=m_cap, cap_kind=cap_kind, garbage=garbage, sub=sub, stop=stop, draw_seed=draw_seed, draw_extra=extra, depth=depth)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return int(np.float32(a).view(np.int32))


def _score_tol(x, y, c, ev):
    """e of the module docstring for one trial of a trace."""
    p = ev["parts"]
    if p["den"] == 0.0:
        return 0.0
    if not np.isfinite(ev["s"]):
        return np.inf
    inl, k = ev["inl"], ev["k"]
    with np.errstate(over="ignore", invalid="ignore"):
        yi, xi = y[inl], x[inl]
        s_c = float(((yi.astype(np.float64) - float(c)) ** 2).sum())
        num32 = float(((yi - xi * ev["a"]).astype(np.float64) ** 2).sum())
    num, den = p["num"], p["den"]
    d_num = abs(num32 - num) + (k + 2) * EPS * max(num32, num)
    d_den = 2 * (k + 4) * EPS * s_c
    if not d_den < den:
        return np.inf
    return d_num / den + num * d_den / (den * (den - d_den)) + 2 * EPS * (1 + abs(ev["s"]))


def _other_slope(q):
    """The neighbouring float32 where the float64 quotient q lies within 2^-40 relative of a float32 rounding boundary, else None."""
    if q is None or q == 0.0 or not np.isfinite(q):
        return None
    with np.errstate(over="ignore"):
        a = np.float32(q)
    if not np.isfinite(a):
        return None
    nb = np.nextafter(a, np.float32(np.inf if q > float(a) else -np.inf))
    if not np.isfinite(nb):
        return None
    mid = (float(a) + float(nb)) / 2
    return nb if abs(q - mid) <= 2.0 ** -40 * abs(q) else None


def _ambiguities(x, y, c, trace, T):
    """[(kind, trial, value)] of one walk: the steps of it that hang on float64 rounding."""
    out, by_t = [], {ev["t"]: ev for ev in trace}
    for ev in trace:
        nb = _other_slope(ev["q"])
        if nb is not None:
            out.append(("slope", ev["t"], nb if _bits(ev["a"]) != _bits(nb) else np.float32(ev["q"])))
        if ev["s"] is not None and ev["best"] >= 0 and ev["k"] == ev["k_best"] and _bits(ev["a"]) != _bits(ev["a_best"]):
            s, sb = ev["s"], ev["score_best"]
            if not (np.isnan(s) or np.isnan(sb)):
                tol = 2 * (_score_tol(x, y, c, ev) + _score_tol(x, y, c, by_t[ev["best"]]))
                if tol > 0 and not abs(s - sb) > tol:
                    out.append(("flip", ev["t"], None))
        q = ev["limit_q"]
        if ev["accepted"] and q is not None and np.isfinite(q) and q > 0:
            r = float(np.round(q))
            if 1 <= r <= T and abs(q - r) <= 1e-9 * r and not ev["limit_same"]:
                out.append(("limit", ev["t"], r + 1 if q <= r else r))
    return out


def _same_result(a, b):
    return all(a[k] == b[k] for k in FIELDS if k != "coef") and (_bits(a["coef"]) == _bits(b["coef"]) or (np.isnan(a["coef"]) and np.isnan(b["coef"])))


def frame_oracle(x, y, count, n_cap, sub, min_samples, T, stop, max_walks=24):
    """One frame: dict(res, alts, undecided, causes, thr0, feats) - the restatement's result, every result another answer to an
    ambiguous step leads to, and what the frame exercises (conditions on the inputs and on the oracle's own walk)."""
    fail = dict(status=R.FAILED, coef=np.float32("nan"), n_inliers=0, n_trials=0, best_trial=-1)
    if count < 0 or count > n_cap:
        return dict(res=fail, alts=[fail], undecided=False, causes=set(), thr0=False, feats={"status 2"})
    x, y = x[:count], y[:count]
    trace = []
    res = R.ransac_scale(x, y, sub, min_samples, T, stop, trace=trace)
    feats, causes, alts, thr0 = {f"status {res['status']}"}, set(), [res], False
    if trace:
        c = np.median(y)
        thr0 = float(R.threshold(y)) == 0.0
        ysort, dsort = np.sort(y), np.sort(np.abs(y - c))
        if count % 2 == 0:
            feats.add("median of y: the upper middle value " + ("differs" if ysort[count // 2] != ysort[count // 2 - 1] else "is equal"))
            feats.add("median of |y - med|: the upper middle value " + ("differs" if dsort[count // 2] != dsort[count // 2 - 1] else "is equal"))
        if thr0:
            feats.add("thr == 0: " + ("fits" if res["status"] == R.OK else "fails"))
        for ev in trace:
            if ev["k"] < 2:
                feats.add("a trial with k < 2")
            elif ev["parts"] and ev["parts"]["den"] == 0.0:
                feats.add("a trial whose inlier y are all equal")
            if ev["q"] is None:
                feats.add("a subset with sum xx == 0")
            if ev["accepted"] and ev["limit_q"] == 0:
                feats.add("trial limit 0")
            if ev["accepted"] and ev["limit_q"] == np.inf:
                feats.add("trial limit infinite")
        if res["status"] == R.OK:
            feats.add("early stop" if res["n_trials"] < T else "all trials run")
        todo, seen = [({}, trace)], {frozenset()}
        while todo and len(seen) <= max_walks:
            state, tr = todo.pop()
            for kind, t, val in _ambiguities(x, y, c, tr, T):
                if not state:
                    causes.add("score" if kind == "flip" else kind)
                if (kind, t) in state:
                    continue
                new = dict(state); new[(kind, t)] = val
                key = frozenset(new)
                if key in seen:
                    continue
                seen.add(key)
                alt = dict(flip={t_ for (k_, t_) in new if k_ == "flip"}, slope={t_: v for (k_, t_), v in new.items() if k_ == "slope"},
                           limit={t_: v for (k_, t_), v in new.items() if k_ == "limit"})
                tr2 = []
                r2 = R.ransac_scale(x, y, sub, min_samples, T, stop, trace=tr2, alt=alt)
                if not any(_same_result(r2, a) for a in alts):
                    alts.append(r2)
                todo.append((new, tr2))
    return dict(res=res, alts=alts, undecided=bool(causes), causes=causes, thr0=thr0, feats=feats)


def expected(c):
    frames = [frame_oracle(c["x"][p], c["y"][p], int(c["counts"][p]), c["n_cap"], c["sub"][p], c["min_samples"], c["T"], c["stop"])
              for p in range(c["P"])]
    depth = None
    d = c["depth"]
    if d is not None:
        sel = [(d["rel"][p][d["valid"][p]], d["met"][p][d["valid"][p]]) for p in range(d["P"])]
        n_cap = d["H"] * d["W"]
        depth = dict(sel=sel, frames=[frame_oracle(sel[p][0], sel[p][1], d["ns"][p], n_cap, d["sub"][p], d["min_samples"], d["T"], 0.99)
                                      for p in range(d["P"])])
    return dict(frames=frames, depth=depth)


_WANT = {}


def oracle_case(seed):
    if seed not in _WANT:
        if len(_WANT) > 64:
            _WANT.clear()
        _WANT[seed] = expected(make_case(seed))
    return _WANT[seed]


def features(c, want):
    """What a case covers, as strings (tests/test_differential_checkers.py::test_align_ransac_slice_covers)."""
    f = {f"P = {c['P']}", f"max_trials {c['T']}", f"stop_probability {c['stop']}", f"min_samples {c['kind']}", f"m_cap {c['cap_kind']}",
         "garbage behind m" if c["garbage"] and c["cap_kind"] == "wide" else "-1 behind m"}
    for p, fw in enumerate(want["frames"]):
        f |= fw["feats"] | {f"family {c['fam'][p]}"}
        if c["fam"][p] not in ("count 0", "count exceeds the row"):
            seg = -(-c["ns"][p] // SEG)
            f |= {f"n = {c['ns'][p]}", f"segments {seg if seg < 5 else '>= 5'}"}
        if c["cap_kind"] == "short" and 1 <= c["ms"][p] <= c["ns"][p] and c["ms"][p] > c["m_cap"]:
            f.add("a frame whose m exceeds m_cap")
        if c["ms"][p] > c["ns"][p] and c["fam"][p] not in SPECIAL:
            f.add("a frame with m > n")
        if c["ms"][p] == c["ns"][p] >= 2:
            f.add("a frame with m == n")
        f |= {f"undecided: {k}" for k in fw["causes"]}
    f |= {f"draw-only n = {n}" for n in c["draw_extra"]}
    d = c["depth"]
    if d is not None:
        f |= {f"depth {d['H']}x{d['W']}", "depth mask" if d["mask"] is not None else "depth without mask"}
        f |= {f"depth status {fw['res']['status']}" for fw in want["depth"]["frames"]}
    return f


# ---- GPU runs -----------------------------------------------------------------------------------------------------------------------
RUNS = [dict(),                      # explicit subsets, one batched call: the default run
        dict(form="single"),         # every frame alone (P = 1): the batched run bit for bit
        dict(form="again"),          # the same call once more: bit for bit
        dict(form="shifted"),        # sample and subset buffers at a base that is 4-byte but not 16-byte aligned: bit for bit
        dict(entry="seeded"),        # subsets drawn on the device from a seed, and the fit fed ransac_subsets(seed)
        dict(entry="draw"),          # ransac_subsets alone, with the draw-only sizes
        dict(entry="chain")]         # align_select_batch / align_depth_batch on the (Pd, H, W) frames


def applies(c, r):
    if r.get("form") == "single":
        return c["P"] > 1
    if r.get("entry") == "chain":
        return c["depth"] is not None
    return True


def _host(res):
    return {k: getattr(res, k).cpu().numpy().copy() for k in FIELDS}


def run_gpu(c, r, cache=None):
    import torch

    from labelany3d_amd import align_depth_batch, ransac_scale_batch, ransac_subsets
    from labelany3d_amd.depth_align import align_select_batch

    cache = {} if cache is None else cache
    dev = torch.device("cuda", torch.cuda.current_device())
    if "x" not in cache:
        cache.update(x=torch.from_numpy(c["x"]).to(dev), y=torch.from_numpy(c["y"]).to(dev), cnt=torch.from_numpy(c["counts"]).to(dev),
                     sub=torch.from_numpy(c["sub"]).to(dev))
    x, y, cnt, sub = cache["x"], cache["y"], cache["cnt"], cache["sub"]
    ms, T, stop = c["min_samples"], c["T"], c["stop"]
    entry, form = r.get("entry"), r.get("form")
    if entry is None and form in (None, "again"):
        return _host(ransac_scale_batch(x, y, cnt, ms, T, subsets=sub, stop_probability=stop))
    if form == "single":
        rows = [_host(ransac_scale_batch(x[p:p + 1], y[p:p + 1], cnt[p:p + 1], ms, T, subsets=sub[p:p + 1], stop_probability=stop))
                for p in range(c["P"])]
        return {k: np.concatenate([g[k] for g in rows]) for k in FIELDS}
    if form == "shifted":
        def shifted(a):
            buf = torch.empty(a.numel() + 1, dtype=a.dtype, device=dev)
            v = buf[1:].view(a.shape)
            v.copy_(a)
            assert v.data_ptr() % 16 == 4
            return v
        return _host(ransac_scale_batch(shifted(x), shifted(y), cnt, ms, T, subsets=shifted(sub), stop_probability=stop))
    if entry == "seeded":
        drawn = ransac_scale_batch(x, y, cnt, ms, T, subsets=None, seed=c["draw_seed"], stop_probability=stop)
        exported = ransac_subsets(cnt, ms, T, seed=c["draw_seed"])
        fed = ransac_scale_batch(x, y, cnt, ms, T, subsets=exported, stop_probability=stop)
        return dict(drawn=_host(drawn), fed=_host(fed), subsets=exported.cpu().numpy())
    if entry == "draw":
        got = dict(subsets=ransac_subsets(cnt, ms, T, seed=c["draw_seed"]).cpu().numpy(), extra=None)
        if c["draw_extra"]:
            got["extra"] = ransac_subsets(np.asarray(c["draw_extra"], np.int64), ms, DRAW_ONLY_TRIALS, seed=c["draw_seed"]).cpu().numpy()
        return got
    if entry == "chain":
        d = c["depth"]
        rel, met = torch.from_numpy(d["rel"]).to(dev), torch.from_numpy(d["met"]).to(dev)
        mask = None if d["mask"] is None else torch.from_numpy(d["mask"]).to(dev)
        ro, mo, n = align_select_batch(rel, met, mask, d["cap"])
        out, res = align_depth_batch(rel, met, mask, d["min_samples"], d["cap"], subsets=torch.from_numpy(d["sub"]).to(dev), max_trials=d["T"])
        return dict(_host(res), out=out.cpu().numpy(), counts=n.cpu().numpy(), rel_sel=ro.cpu().numpy(), met_sel=mo.cpu().numpy())
    raise ValueError(r)


# ---- the checker --------------------------------------------------------------------------------------------------------------------
def ulp_apart(a, b):
    """Equal or adjacent float32 (tests/test_gpu_align_ransac.py::_ulp_apart)."""
    a, b = np.float32(a), np.float32(b)
    return bool(a == b or np.nextafter(a, b) == b)


def ulp_distance(a, b):
    def key(v):
        i = int(np.float32(v).view(np.int32))
        return i if i >= 0 else -(i & 0x7fffffff)
    return abs(key(a) - key(b))


def _matches(g, w):
    if any(int(g[k]) != int(w[k]) for k in FIELDS if k != "coef"):
        return False
    if w["status"] != R.OK:
        return bool(np.isnan(g["coef"]))
    return bool(np.isfinite(g["coef"])) == bool(np.isfinite(w["coef"])) and (ulp_apart(g["coef"], w["coef"]) or
                                                                             (np.isnan(g["coef"]) and np.isnan(w["coef"])))


def check_frame(fw, g, tally=None):
    """One frame's five fields against its oracle: exactly (coef to the adjacent float32) where the frame is decided, against every walk
    of the loop the oracle accepts where it is not."""
    w = fw["res"]
    if int(g["status"]) != w["status"]:
        return [f"status {int(g['status'])}, oracle {w['status']}"]
    for a in (fw["alts"] if fw["undecided"] else [w]):
        if _matches(g, a):
            if tally is not None and a["status"] == R.OK and np.isfinite(a["coef"]) and np.isfinite(g["coef"]):
                tally["worst_ulp"] = max(tally["worst_ulp"], ulp_distance(g["coef"], a["coef"]))
            return []
    got = {k: (float(g[k]) if k == "coef" else int(g[k])) for k in FIELDS}
    ref = {k: (float(w[k]) if k == "coef" else int(w[k])) for k in FIELDS}
    return [f"{'undecided ' + str(sorted(fw['causes'])) if fw['undecided'] else 'decided'} frame{' (thr == 0)' if fw['thr0'] else ''}: "
            f"got {got}, oracle {ref}" + (f" or one of {len(fw['alts']) - 1} other walks" if fw["undecided"] else "")]


def _fields_equal(a, b):
    return [f"{k} differs in frames {np.flatnonzero(a[k].view(np.int32) != b[k].view(np.int32))[:8].tolist()}" for k in FIELDS
            if a[k].shape != b[k].shape or (a[k].view(np.int32) != b[k].view(np.int32)).any()]


def check_draw(counts, min_samples, sub, T):
    """Every row: m distinct indices in [0, n), then -1 (m == n: a permutation); a frame that cannot be drawn for is all -1."""
    msgs = []
    counts = [int(v) for v in counts]
    ms = [R.subset_size(min_samples, n) if n > 0 else 0 for n in counts]
    ms = [m if 1 <= m <= n else 0 for m, n in zip(ms, counts)]
    if sub.dtype != np.int32 or sub.ndim != 3 or sub.shape[:2] != (len(counts), T):
        return [f"subsets of shape {sub.shape}, dtype {sub.dtype}"]
    for p, (n, m) in enumerate(zip(counts, ms)):
        if m > sub.shape[2]:
            msgs.append(f"frame {p}: m = {m} does not fit the {sub.shape[2]} columns"); continue
        head, tail = sub[p, :, :m], sub[p, :, m:]
        if (tail != -1).any():
            msgs.append(f"frame {p} (n = {n}, m = {m}): an entry behind m is not -1")
        if m and ((head < 0) | (head >= n)).any():
            msgs.append(f"frame {p} (n = {n}, m = {m}): an index outside [0, n)")
        elif m > 1 and (np.diff(np.sort(head, axis=1), axis=1) == 0).any():
            msgs.append(f"frame {p} (n = {n}, m = {m}): a trial draws an index twice")
    return msgs


def _same_or_nan(a, b):
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


def check_run(c, want, r, got, default=None, tally=None):
    msgs = []
    entry, form = r.get("entry"), r.get("form")
    if entry is None:
        for p, fw in enumerate(want["frames"]):
            msgs += [f"frame {p} ({c['fam'][p]}, n = {c['ns'][p]}): {m}" for m in check_frame(fw, {k: got[k][p] for k in FIELDS}, tally)]
        if form is not None:
            msgs += [f"not the batched run bit for bit: {m}" for m in (_fields_equal(got, default) if default is not None else ["no default run"])]
    elif entry == "seeded":
        msgs += [f"the seeded fit is not the fit fed ransac_subsets(seed): {m}" for m in _fields_equal(got["drawn"], got["fed"])]
        sub = got["subsets"]
        bad = check_draw(c["counts"], c["min_samples"], sub, c["T"])
        msgs += bad
        if not bad:
            for p in range(c["P"]):
                fw = frame_oracle(c["x"][p], c["y"][p], int(c["counts"][p]), c["n_cap"], sub[p], c["min_samples"], c["T"], c["stop"])
                if tally is not None:
                    tally["seeded frames"] += 1
                    tally["seeded undecided"] += int(fw["undecided"])
                msgs += [f"frame {p} ({c['fam'][p]}, n = {c['ns'][p]}) on the exported subsets: {m}"
                         for m in check_frame(fw, {k: got["drawn"][k][p] for k in FIELDS}, tally)]
    elif entry == "draw":
        msgs += check_draw(c["counts"], c["min_samples"], got["subsets"], c["T"])
        if c["draw_extra"]:
            msgs += [f"draw-only leg: {m}" for m in check_draw(c["draw_extra"], c["min_samples"], got["extra"], DRAW_ONLY_TRIALS)]
    elif entry == "chain":
        d, wd = c["depth"], want["depth"]
        if got["counts"].tolist() != d["ns"]:
            msgs.append(f"selection counts {got['counts'].tolist()}, expected {d['ns']}")
        for p in range(d["P"]):
            n = d["ns"][p]
            xs, ys = wd["sel"][p]
            if got["counts"][p] == n and not (_same_or_nan(got["rel_sel"][p, :n], xs).all() and _same_or_nan(got["met_sel"][p, :n], ys).all()):
                msgs.append(f"depth frame {p}: the selected samples are not the valid pixels in row-major order")
            bad = check_frame(wd["frames"][p], {k: got[k][p] for k in FIELDS}, tally)
            msgs += [f"depth frame {p} ({d['fam'][p]}, {d['H']}x{d['W']}, n = {n}): {m}" for m in bad]
            if bad:
                continue
            if int(got["status"][p]) == R.OK:
                sel = d["mask"][p] if d["mask"] is not None else ~np.isinf(d["rel"][p])
                with np.errstate(over="ignore", invalid="ignore"):
                    exp = np.where(sel, (d["rel"][p] * np.float32(got["coef"][p])).astype(np.float32), FILL)
                what = "where(sel, float32(rel * coef), 10000)"
            else:
                exp, what = d["met"][p], "the metric depth"
            ne = ~_same_or_nan(np.ascontiguousarray(got["out"][p]), np.ascontiguousarray(exp))
            if ne.any():
                i = tuple(int(v) for v in np.argwhere(ne)[0])
                msgs.append(f"depth frame {p} (status {int(got['status'][p])}): {int(ne.sum())} pixels are not {what}, first at {i}: "
                            f"{got['out'][p][i]!r}, expected {exp[i]!r}")
    return msgs


# ---- tally --------------------------------------------------------------------------------------------------------------------------
def new_tally():
    t = {k: 0 for k in ("cases", "frames", "decided", "undecided", "thr0", "thr0 fitted", "status 0", "status 1", "status 2", "calls",
                        "worst_ulp", "depth frames", "seeded frames", "seeded undecided")}
    t["causes"] = {"score": 0, "limit": 0, "slope": 0}
    return t


def tally_case(t, c, want):
    t["cases"] += 1
    for fw in want["frames"] + (want["depth"]["frames"] if want["depth"] else []):
        t["frames"] += 1
        t["undecided" if fw["undecided"] else "decided"] += 1
        t["thr0"] += int(fw["thr0"])
        t["thr0 fitted"] += int(fw["thr0"] and fw["res"]["status"] == R.OK)
        t[f"status {fw['res']['status']}"] += 1
        for k in fw["causes"]:
            t["causes"][k] += 1
    t["depth frames"] += len(want["depth"]["frames"]) if want["depth"] else 0


def undecided_share(t):
    return t["undecided"] / max(t["frames"], 1)


def tally_lines(t):
    return [f"align_ransac: {t['cases']} cases, {t['frames']} frames ({t['depth frames']} of them depth frames of the chain), {t['calls']} calls",
            f"  decided {t['decided']}, undecided {t['undecided']} ({100 * undecided_share(t):.2f} %; causes: " +
            ", ".join(f"{k} {v}" for k, v in t["causes"].items()) + ")",
            f"  thr == 0: {t['thr0']} frames, {t['thr0 fitted']} of them fitted (held to the restatement like every other frame)",
            f"  status 0 / 1 / 2: {t['status 0']} / {t['status 1']} / {t['status 2']}",
            f"  device-drawn fits checked on their exported subsets: {t['seeded frames']} frames, {t['seeded undecided']} undecided",
            f"  worst coefficient distance: {t['worst_ulp']} ulp"]
