"""The depth gate on bit planes (include/la3d.h "depth gate on bit planes"): the NumPy restatement of the rule - the oracle of
tests/test_depth_gate_contract.py and tests/test_gpu_depth_gate.py - and the case generators, all from ``np.random.RandomState`` seeds.
Nothing here needs a GPU."""
import functools

import numpy as np

INF = float("inf")
FILL = np.float32(10000.0)          # what the reference's align_depth writes where it cannot predict
SENTINEL = 0x5A5A5A5A


def gate(depth, mask, k=4.5, min_band=0.0, near=-INF, far=INF):
    """The rule, per instance: ``depth`` float32 (H, W) and ``mask`` bool (H, W), the image columns only ->
    (keep bool (H, W), counts int32 [3] = area_in, n_valid, area_out, levels float32 [3] = med, mad, thr)."""
    d = np.asarray(depth)
    m = np.asarray(mask, bool)
    assert d.dtype == np.float32 and d.shape == m.shape
    with np.errstate(invalid="ignore", over="ignore"):
        valid = m & np.isfinite(d) & (d >= np.float32(near)) & (d <= np.float32(far))
        v = d[valid]                                                      # float32
        if v.size == 0:
            return np.zeros_like(m), np.array([m.sum(), 0, 0], np.int32), np.full(3, np.nan, np.float32)
        med = np.median(v)                                                # float32; an even count averages the two middle values in float32
        mad = np.median(np.abs(v - med))                                  # float32, same rule
        thr = np.maximum(np.float32(k) * mad, np.float32(min_band))       # one float32 product
        keep = valid & (np.abs(d - med) <= thr)                           # one float32 subtraction per pixel
    assert med.dtype == mad.dtype == thr.dtype == np.float32
    return keep, np.array([m.sum(), valid.sum(), keep.sum()], np.int32), np.array([med, mad, thr], np.float32)


def gate_batch(depths, masks, **kw):
    """``gate`` for a batch -> (keep (B, H, W), counts (B, 3), levels (B, 3))"""
    res = [gate(d, m, **kw) for d, m in zip(depths, masks)]
    if not res:
        H, W = np.shape(masks)[1:]
        return np.zeros((0, H, W), bool), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32)
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res])


def stored_width(W, pad):
    return (W + 31) // 32 * 32 if pad else W


def pack(masks, W_stored):
    """bool (B, H, W) -> the uint32 (B, ceil(H * W_stored / 32)) words of the planes as stored W_stored wide"""
    m = np.asarray(masks, bool)
    B, H, W = m.shape
    full = np.zeros((B, H, W_stored), bool)
    full[:, :, :W] = m
    flat = full.reshape(B, -1)
    nwords = (H * W_stored + 31) // 32
    bits = np.zeros((B, nwords * 32), bool)
    bits[:, :flat.shape[1]] = flat
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(B, nwords)


def not_image(H, W, W_stored):
    """the uint32 words whose set bits are the bits of a stored plane that are NOT image: pad columns and the tail of the last word"""
    nwords = (H * W_stored + 31) // 32
    bits = np.ones(nwords * 32, bool)
    img = np.zeros((H, W_stored), bool)
    img[:, :W] = True
    bits[:H * W_stored] = ~img.reshape(-1)
    return np.packbits(bits, bitorder="little").view(np.uint32)


def pad_depth(depths, W_stored, fill=0.0):
    d = np.asarray(depths, np.float32)
    out = np.full(d.shape[:-1] + (W_stored,), fill, np.float32)
    out[..., :d.shape[-1]] = d
    return out


# ---- generators ------------------------------------------------------------------------------------------------------------------
FRAMES = ((12, 40, False), (12, 37, True), (5, 7, False))      # H, W, frame_pad: unpadded; stored 64; the last word partly outside
BIG = (96, 96)                                                 # 9216 pixels: beyond the 6144 keys the selection holds in LDS

PARAMS = (                                                     # the scalars of a call; the smooth planes have their median near 2.5
    {}, dict(k=0.0), dict(k=1.0, min_band=0.05), dict(k=1.0, min_band=1.0), dict(k=0.0, min_band=0.01),
    dict(near=2.0), dict(near=2.7), dict(far=3.0), dict(far=2.3), dict(far=9999.0), dict(k=2.0, near=-1.0, far=1.0),
)


def smooth(rs, H, W):
    """a tilted surface between 1.5 and 3.5 with a little noise: every depth distinct, the median near 2.5"""
    v, u = np.mgrid[0:H, 0:W]
    return (1.5 + 2.0 * (v * W + u) / max(H * W - 1, 1) + rs.uniform(-0.01, 0.01, (H, W))).astype(np.float32)


def depth_kinds(rs, H, W):
    """name -> float32 (H, W): the depth contents the selection can go wrong on"""
    s = smooth(rs, H, W)
    levels = np.where(rs.rand(H, W) < 0.5, np.float32(2.0), np.float32(2.5)).astype(np.float32)
    ulps = (np.float32(2.0).view(np.uint32) + rs.randint(0, 16, (H, W)).astype(np.uint32)).view(np.float32)   # all but the lowest mantissa bits shared
    bad = s.copy()
    flat = bad.reshape(-1)
    idx = rs.permutation(flat.size)[:max(4, flat.size // 6)]
    flat[idx] = np.resize(np.array([np.nan, np.inf, -np.inf, FILL], np.float32), idx.size)
    return dict(smooth=s, constant=np.full((H, W), 2.25, np.float32), levels=levels, ulps=ulps, negative=-s,
                mixed=(s - np.float32(2.5)).astype(np.float32), invalid=bad)


def mask_kinds(rs, H, W):
    """name -> bool (H, W): empty, one pixel, two pixels, an odd and an even count, the full frame, a random half"""
    def some(n):
        m = np.zeros(H * W, bool)
        m[rs.permutation(H * W)[:n]] = True
        return m.reshape(H, W)
    return dict(empty=np.zeros((H, W), bool), one=some(1), two=some(2), odd=some(min(21, H * W - (H * W + 1) % 2)),
                even=some(min(22, H * W - H * W % 2)), full=np.ones((H, W), bool), half=rs.rand(H, W) < 0.5)


@functools.lru_cache(maxsize=None)
def planes(H, W, seed=0):
    """-> (names, depths float32 (B, H, W), masks bool (B, H, W)): every mask kind on the smooth surface, every depth kind under the
    full frame and under a random half"""
    rs = np.random.RandomState(1000 * H + W + seed)
    dk, mk = depth_kinds(rs, H, W), mask_kinds(rs, H, W)
    names, depths, masks = [], [], []
    for mn, m in mk.items():
        names.append(f"smooth/{mn}"); depths.append(dk["smooth"]); masks.append(m)
    for dn, d in dk.items():
        if dn == "smooth":
            continue
        for mn in ("full", "half"):
            names.append(f"{dn}/{mn}"); depths.append(d); masks.append(mk[mn])
    depths, masks = np.stack(depths), np.stack(masks)
    depths.setflags(write=False); masks.setflags(write=False)
    return tuple(names), depths, masks


@functools.lru_cache(maxsize=None)
def big_planes(seed=7):
    """-> (names, depths, masks) of 96 x 96: full masks over the depth contents that drive both selection paths - smooth (the sample
    brackets the median), constant (all ties), two levels at 50 / 50 and 49 / 51, shared mantissas, negative and mixed signs, invalid
    pixels - and smooth planes whose valid counts lie on both sides of the 6144 keys the LDS buffer holds"""
    H, W = BIG
    rs = np.random.RandomState(seed)
    dk = depth_kinds(rs, H, W)
    n = H * W
    order = rs.permutation(n)

    def two_levels(share):
        d = np.full(n, 2.5, np.float32)
        d[order[:int(round(n * share))]] = np.float32(2.0)
        return d.reshape(H, W)

    def count(c):
        m = np.zeros(n, bool)
        m[order[:c]] = True
        return m.reshape(H, W)

    full = np.ones((H, W), bool)
    rows = [(name, d, full) for name, d in dk.items()]
    rows += [("levels_50_50", two_levels(0.5), full), ("levels_49_51", two_levels(0.49), full), ("levels_51_49", two_levels(0.51), full)]
    rows += [(f"count_{c}", dk["smooth"], count(c)) for c in (6143, 6144, 6145, 6146, 9215)]
    rows += [("levels_count_6145", two_levels(0.5), count(6145)), ("constant_count_6146", dk["constant"], count(6146))]
    depths, masks = np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows])
    depths.setflags(write=False); masks.setflags(write=False)
    return tuple(r[0] for r in rows), depths, masks


@functools.lru_cache(maxsize=None)
def expected(which, params_index):
    """the restatement on ``planes(*which)`` (or ``big_planes()`` for which == "big") under PARAMS[params_index], computed once"""
    _, depths, masks = big_planes() if which == "big" else planes(*which)
    return gate_batch(depths, masks, **PARAMS[params_index])


def scene():
    """The case the feature exists for -> (depth float32 (48, 64), mask bool (48, 64)): a rectangular mask at 2 m +- 5 cm, a
    four-column strip of it at 7.5 m (the wall behind the object) and one pixel of the depth stage's fill value."""
    rs = np.random.RandomState(48064)
    H, W = 48, 64
    depth = np.full((H, W), 7.5, np.float32)
    mask = np.zeros((H, W), bool)
    mask[8:40, 10:50] = True
    depth[8:40, 10:46] = (2.0 + rs.uniform(-0.05, 0.05, (32, 36))).astype(np.float32)
    depth[20, 30] = FILL
    return depth, mask
