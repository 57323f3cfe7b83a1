"""The inputs of the 16-bit depth tests (include/la3d.h "16-bit depth planes"), shared by tests/test_depth16_contract.py - which shows
on the CPU that the oracle alone passes every comparison - and tests/test_gpu_depth16.py.  Planes are quantised HERE with NumPy
(``astype(np.float16)``, the ``rint`` rule), never with the packer under test, and up-converted by the value rule of the header."""
import numpy as np

from oracle import la3d_oracle as O
from oracle import poly_oracle as P

K224 = np.array([[180.0, 0, 112], [0, 180.0, 48], [0, 0, 1]])
K640 = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
NSAMPLE = 500

# (dtype, scale, zero_is_hole): both products float32(x) * scale are inexact for these scales
VARIANTS = [("f16", 1.0, True), ("u16", 0.001, True), ("u16", 0.00025, False)]
VARIANT_IDS = ["f16", "u16-mm-hole", "u16-quarter-mm"]


def quantise(d32, dtype, scale=0.001):
    """float32 depth -> the stored 16-bit planes: astype(float16), or q = rint(d / scale) in float32 with NaN, +-inf and d <= 0 -> 0
    and q > 65535 -> 65535 (the rule of la3d_pack_depth16)"""
    d32 = np.asarray(d32, np.float32)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return d32.astype(np.float16)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = np.rint(d32 / np.float32(scale))
        q = np.where(np.isfinite(d32) & (d32 > 0), np.minimum(q, np.float32(65535)), np.float32(0))
    return q.astype(np.uint16)


def upconvert(x, scale=1.0, hole=True):
    """the float32 value the kernels fit for the stored planes x (the definition every test uses)"""
    x = np.asarray(x)
    if x.dtype == np.float16:
        return x.astype(np.float32)
    assert x.dtype == np.uint16
    v = x.astype(np.float32) * np.float32(scale)
    return np.where((x == 0) & bool(hole), np.float32("nan"), v).astype(np.float32)


def blob_masks(rs, B, H, W):
    """rectangles, an ellipse, 2 % random pixels, one empty mask (status 1) - the mix of tests/test_gpu_masks.py"""
    masks = np.zeros((B, H, W), bool)
    for i in range(B - 3):
        h, w = rs.randint(6, max(7, min(301, H + 1))), rs.randint(6, max(7, min(331, W + 1)))
        h, w = min(h, H), min(w, W)
        r0, c0 = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
        masks[i, r0:r0 + h, c0:c0 + w] = True
    vv, uu = np.mgrid[0:H, 0:W]
    masks[B - 3] = ((uu - 0.47 * W) ** 2 / (0.15 * W) ** 2 + (vv - 0.42 * H) ** 2 / (0.13 * H) ** 2) < 1.0
    masks[B - 2] = rs.rand(H, W) < 0.02
    return masks


def smooth_depth(rs, P, H, W):
    """sloped planes with 0.05 m noise, 2 .. 9 m: every value survives either quantisation as a positive depth"""
    vv, uu = np.mgrid[0:H, 0:W]
    return (2.0 + rs.uniform(0, 3, (P, 1, 1)) + 0.004 * uu[None] + 0.006 * vv[None] + 0.05 * rs.randn(P, H, W)).astype(np.float32)


def ground_rows(rs, B):
    return np.array([[0.02, -0.98, 0.1, 1.5]] * B) + 0.03 * rs.randn(B, 4)


def ellipse_segs(rs, B, H, W):
    segs = []
    for _ in range(B):
        cy, cx = rs.uniform(0.3, 0.7) * H, rs.uniform(0.3, 0.7) * W
        ry, rx = rs.uniform(0.12, 0.26) * H, rs.uniform(0.12, 0.26) * W
        t = np.linspace(0, 2 * np.pi, 20, endpoint=False)
        segs.append([np.stack([cx + rx * np.cos(t), cy + ry * np.sin(t)], 1).reshape(-1).tolist()])
    return segs


def hull_masks(rs, B, H, W, rmax=0.2):
    """elliptic masks small enough for the column arrays of a full-mask hull call (tests/test_gpu_hull_instances.py: hull_scene)"""
    vv, uu = np.mgrid[0:H, 0:W]
    masks = np.zeros((B, H, W), bool)
    for n in range(B):
        cy, cx = rs.uniform(0.25, 0.75) * H, rs.uniform(0.25, 0.75) * W
        ry, rx = rs.uniform(0.09, rmax) * H, rs.uniform(0.09, rmax) * W
        masks[n] = ((vv - cy) / ry) ** 2 + ((uu - cx) / rx) ** 2 <= 1.0
    return masks


def draw_sample_idx(counts, rs):
    idx = np.zeros((len(counts), NSAMPLE), np.int32)
    for n, c in enumerate(counts):
        if c > NSAMPLE:
            idx[n] = rs.randint(0, int(c), NSAMPLE)
    return idx


def _case(name, d32, masks, K, ground=None, sample=False, method="pca", ii=None, entry="u8", segs=None, special=None, empty=(),
          seed=0):
    """``special(stored, masks, dtype, hole)``: writes special values into the STORED planes and returns {instance: expected status}"""
    return dict(name=name, d32=d32, masks=masks, K=K, ground=ground, sample=sample, method=method, ii=ii, entry=entry, segs=segs,
                special=special, empty=tuple(empty), seed=seed)


def _under(masks, n, k):
    r, c = np.argwhere(masks[n])[k]
    return int(r), int(c)


def special_checked(stored, masks, dtype, hole):
    """the checked pass: NaN, +inf, a negative value and -0 under the mask (float16); holes (uint16: stored 0)"""
    if dtype == "f16":
        for n, v in ((0, np.nan), (1, np.inf), (2, -2.0), (3, -0.0)):
            r, c = _under(masks, n, 7)
            stored[n if len(stored) > 1 else 0, r, c] = np.float16(v)
    else:
        for n in range(4):
            r, c = _under(masks, n, 7)
            stored[n if len(stored) > 1 else 0, r, c] = 0
    return {}


def special_values(stored, masks, dtype, hole):
    """float16: smallest subnormal, 65504, inf, NaN; uint16: 0 and 65535 under the mask (0 is a hole with the flag, the valid depth 0.0
    without it); instance 4: only NaN / only holes -> the status of an all-NaN instance (1).  Without the flag instance 4 stays as it
    is: a mask of depths 0.0 has no spread at all, the suite's documented don't-care."""
    vals = [np.float16(6e-8), np.float16(65504), np.float16(np.inf), np.float16(np.nan)] if dtype == "f16" else [0, 65535, 0, 65535]
    for n, v in enumerate(vals):
        for k in (5, 11):
            r, c = _under(masks, n, k)
            if n == 1:
                # the largest value sits next to the principal point (48, 112) of K224: its point is (~0, ~0, d), so no corner of the
                # box passes 65504 and the record's float16-quantised vertices stay finite (a corner beyond overflows to inf, then
                # inf * 0 = NaN in the un-rotation - in the reference's own arithmetic: nothing a comparison could be held to)
                r, c = 48, 112 + (k == 11)
                assert masks[n, r, c]
            stored[n, r, c] = v
    if dtype == "f16" or hole:
        stored[4][masks[4]] = np.float16(np.nan) if dtype == "f16" else 0
        return {4: 1}
    return {}


def fixed_cases():
    """Every fixed case of the GPU file, by name.  Shapes: 96 x 224 (84 tiles, tiled), 100 x 224 (H & 7 != 0), 64 x 96 (24 tiles,
    untiled), 100 x 214 and 61 x 75 (W % 32 != 0; at 75 a 16-bit row starts on 2-byte boundaries only), 480 x 640 with B = 24."""
    cases = []
    shapes = [(96, 224), (100, 224), (64, 96), (100, 214), (61, 75)]
    for H, W in shapes:
        rs = np.random.RandomState(H * 1000 + W)
        B = 10
        K = K224.copy()
        K[0, 2], K[1, 2] = W / 2, H / 2
        masks = blob_masks(rs, B, H, W)
        d = smooth_depth(rs, B, H, W)
        tag = f"{W}x{H}"
        cases.append(_case(f"sep {tag}", d, masks, K, empty=[B - 1]))                                      # separable single pass
        Ks = K.copy(); Ks[0, 1] = 2.5
        cases.append(_case(f"ground {tag}", d, masks, K, ground=ground_rows(rs, B), empty=[B - 1]))        # two passes
        cases.append(_case(f"skew {tag}", d, masks, Ks, empty=[B - 1]))
        cases.append(_case(f"checked {tag}", d, masks, K, special=special_checked, empty=[B - 1]))
        cases.append(_case(f"checked ground {tag}", d, masks, K, ground=ground_rows(rs, B), special=special_checked, empty=[B - 1]))
        sm = masks.copy()
        for n in (2, 5):   # masks of at most 500 pixels: not sampled
            sm[n] = False
            sm[n, 10:10 + 9 + n, 12:40] = True
        cases.append(_case(f"subsample {tag}", d, sm, K, ground=ground_rows(rs, B), sample=True, empty=[B - 1], seed=H + W))
        # pivot pass: footprints 2 px wide at ~60 m (kappa = (distance / spread)^2 ~ 1e6 > 2^17), depth stepping by the float16 quantum
        pm = np.zeros((6, H, W), bool)
        for n in range(6):
            c0 = 5 + 11 * n
            pm[n, 8:8 + 30 + n, c0:c0 + 2] = True
        vv = np.mgrid[0:H, 0:W][0]
        pd = np.broadcast_to((60.0 + 0.03125 * (vv % 5)).astype(np.float32), (6, H, W)).copy()
        cases.append(_case(f"pivot {tag}", pd, pm, K640 if W >= 214 else K224 * [[3], [3], [1]]))
    # hull: full-mask on the tiled frame (84 tiles: masks of at most 28 active tiles), subsample mode with ground anywhere
    for H, W in [(96, 224), (100, 214)]:
        rs = np.random.RandomState(77 + W)
        B = 8
        K = np.array([[0.8 * W, 0, W / 2.0], [0, 0.8 * W, H / 2.0], [0, 0, 1]])
        hm = hull_masks(rs, B, H, W)
        d = smooth_depth(rs, B, H, W)
        cases.append(_case(f"hull full {W}x{H}", d, hm, K, method="convex_hull", entry="u8" if W % 32 == 0 else "rle"))
        bm = hull_masks(rs, B, H, W, rmax=0.3)
        bm[2] = False; bm[2, 20:32, 30:60] = True
        cases.append(_case(f"hull subsample {W}x{H}", d, bm, K, ground=ground_rows(rs, B), sample=True, method="convex_hull", seed=W))
    # every mask source at 96 x 224 and (padded rows: frame_width) at 100 x 214
    for H, W in [(96, 224), (100, 214)]:
        rs = np.random.RandomState(31 + W)
        B = 8
        K = K224.copy()
        d = smooth_depth(rs, B, H, W)
        masks = blob_masks(rs, B, H, W)
        for entry in ("rle", "bits"):
            cases.append(_case(f"{entry} {W}x{H}", d, masks, K, entry=entry, empty=[B - 1]))
            cases.append(_case(f"{entry} ground {W}x{H}", d, masks, K, ground=ground_rows(rs, B), entry=entry, empty=[B - 1]))
        segs = ellipse_segs(rs, B, H, W)
        pmask = np.stack([P.create_boolean_mask_from_polygon((W, H), s)[0] for s in segs]).astype(bool)
        cases.append(_case(f"poly {W}x{H}", d, pmask, K, entry="poly", segs=segs))
        cases.append(_case(f"poly ground {W}x{H}", d, pmask, K, ground=ground_rows(rs, B), entry="poly", segs=segs))
    # special values, one instance per plane
    rs = np.random.RandomState(5)
    H, W, B = 96, 224, 8
    masks = blob_masks(rs, B, H, W)
    masks[B - 1] = masks[0]
    masks[1] = False
    masks[1, 30:70, 90:140] = True                                    # holds the principal point (see special_values)
    d = smooth_depth(rs, B, H, W)
    cases.append(_case("special values", d, masks, K224, special=special_values))
    cases.append(_case("special values ground", d, masks, K224, ground=ground_rows(rs, B), special=special_values))
    # the large frame: 1200 tiles - cull plan and kept tiles in the two-pass form
    rs = np.random.RandomState(640)
    H, W, B, Pn = 480, 640, 24, 3
    masks = blob_masks(rs, B, H, W)
    d = smooth_depth(rs, Pn, H, W)
    ii = (np.arange(B) % Pn).astype(np.int32)
    Ks = np.stack([K640, K640 * [[1.1], [0.9], [1]], K640 * [[0.9], [1.2], [1]]])
    Ks[2, 0, 1] = 2.5
    cases.append(_case("640x480 sep + skew, shared planes", d, masks, Ks, ii=ii, empty=[B - 1]))
    cases.append(_case("640x480 ground, shared planes", d, masks, Ks, ground=ground_rows(rs, B), ii=ii, empty=[B - 1]))
    return cases


def materialise(case, variant):
    """(stored planes, up-converted float32 planes, expected status per instance, sample_idx) of a case for one (dtype, scale, hole)"""
    dtype, scale, hole = variant
    stored = quantise(case["d32"], dtype, scale)
    masks = case["masks"]
    B = len(masks)
    want = np.zeros(B, np.int64)
    for n in case["empty"]:
        want[n] = 1
    if case["special"] is not None:
        for n, st in case["special"](stored, masks, dtype, hole).items():
            want[n] = st
    up = upconvert(stored, scale, hole)
    sidx = None
    if case["sample"]:
        sidx = draw_sample_idx(masks.reshape(B, -1).sum(1), np.random.RandomState(1000 + case["seed"]))
    return stored, up, want, sidx


def oracle_gaps(up, masks, K, ground=None, sample_idx=None, depth_index=None, method="pca"):
    """(status, eigen-gap) per instance from the oracle (O.fit_points' aux)"""
    K = np.asarray(K, np.float64)
    st, gap = np.zeros(len(masks), np.int64), np.full(len(masks), np.nan)
    for n in range(len(masks)):
        img = int(depth_index[n]) if depth_index is not None else (n if up.shape[0] > 1 else 0)
        pts = O.depth_to_points(up[img][None], K[img] if K.ndim == 3 else K)[masks[n]]
        ri = np.asarray(sample_idx[n]) if (sample_idx is not None and len(pts) > NSAMPLE) else False
        _, st[n], aux = O.fit_points(pts, None if ground is None else ground[n], ri, method)
        gap[n] = aux.get("gap", np.nan)
    return st, gap
