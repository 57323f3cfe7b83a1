"""The randomised differential campaign over the instance point clouds (la3d_instance_point_offsets / la3d_gather_instance_points,
labelany3d_amd/csrc/la3d_cloud.hip; instance_points / instance_points_frames, labelany3d_amd/clouds.py): case generator, oracle, GPU
runs and the checker.  profiles/clouds/fuzz_clouds.py drives it at scale; tests/test_gpu_differential.py runs a committed slice of its
seeds (tests/campaign_slices.py::CLOUD_SEEDS).

One CASE = P images, each with its own size, B instances with masks, image_index, one camera per image and - in about 40 % of the
cases - sample_idx.  In about 60 % of the cases all images share one size and every run of RUNS applies; the rest are mixed and only
the frames runs apply.  The frames are the smallest at which the kernels can still go wrong, aimed at the limits of la3d_cloud.hip:
  band capacity     a band's bit image holds BAND_PIX = 65536 pixels = 1024 words of 64, scanned four words per thread: 1x65536,
                    3x65536, 4x16384 (full bands), 2x65535 (1024 words, the last one short), 2x65520 (padded to a pitch of 65536 in
                    the frames form), all with B <= 3; bands(B, H, W) restates cloud_bands, so masks can aim at a band's first and
                    last pixel and at runs across a band's first row
  scan chunks       cloud_scan_kernel gives each of 1024 threads ceil(B / 1024) instances: B = 1025 (chunk 2, half the threads idle),
                    2049 and 2500 (chunk 3, a ragged last run) on frames of at most 9x40, and one 33x47 case with B = 2049
  select width      masks of one pixel per 4096 on the capacity frames: a select that searches the whole word table
  tiny, odd frames  1x1, 1x333, 1000x1 (bands of 16 pixels and a last one of 8: both u8 forms in one instance), 5x13, 33x47, 40x70,
                    30x40, 96x224, 100x214; at most one 480x640 image (B <= 3): the one band split with trailing empty bands
  u8 bytes          1, 0xff, or a random one of 1 / 2 / 0x80 / 0xff per pixel
  depth             planes with NaN, +-inf, 0 and negative depths; 16-bit runs quantise them HERE with NumPy (quantise / upconvert:
                    the value rule of include/la3d.h "16-bit depth planes"), never with the packer
  sample_idx        drawn as draw_sample_idx draws it, plus hand-made rows (repeated ranks, -1, N, N - 1), instances of exactly 500
                    and 501 pixels, garbage in the rows of instances the rule leaves whole

expected(c) is the oracle: per instance O.depth_to_points(depth[img][None], K[img]) at the mask's pixels in row-major order, the
500-row rule, NaN rows with pixel -1 for ranks outside the cloud, a frame_width below W.  check_run holds every run to it:
  exact (NaN equal to NaN, no waiver)   counts, offsets, status, pixels; every row equal to the la.unproject row of its pixel (the
                    documented bit-for-bit contract); float32 output equal to the cast of the float64 run; bit-plane and frames runs
                    equal to the default run's rows; a short capacity: status 1 and untouched rows for every instance whose range ends
                    beyond it, nothing written at or beyond offsets[-1]
  rtol = atol = 1e-13   points against the oracle (the figure of tests/test_gpu_parity.py for unproject); 16-bit runs against the oracle
                    on the NumPy-upconverted planes
Left out on purpose: masks that change between the two stages and graph capture (tests/test_gpu_instance_points.py has both; neither is
a function of the inputs alone).

The oracle is test infrastructure: it is the checker here."""
import numpy as np

NSAMPLE = 500
BAND_PIX = 65536       # pixels of a band's bit image (la3d_cloud.hip)
MAX_BANDS = 64
WANT_WGS = 8192
SCAN_THREADS = 1024    # threads of cloud_scan_kernel
TOL = 1e-13            # tests/test_gpu_parity.py: unproject against the oracle
SENT = -12345.0        # what the output buffers of a short-capacity run hold before the call

TINY = [(1, 1), (1, 333), (1000, 1), (5, 13), (33, 47), (40, 70), (30, 40), (96, 224), (100, 214)]
CAPACITY = [(1, 65536), (3, 65536), (2, 65535), (4, 16384), (2, 65520)]
BIG = (480, 640)
SMALL = [(9, 40), (7, 33), (3, 5), (8, 32)]       # the frames of the large batches
BS = [1, 2, 3, 7, 33, 300]
LARGE_BS = [1025, 2049, 2500]
SCALES = [0.001, 0.00025, 0.0025, 0.0001]          # (0.0001: depths above 6.5535 m saturate at 65535 units)
DEPTH_KINDS = ("f32", "f16", "u16h", "u16n")


# ------------------------------------------------------------------------------------------------------------------------------
# the band split of la3d_cloud.hip, restated
# ------------------------------------------------------------------------------------------------------------------------------
def padded_width(W):
    return (W + 31) // 32 * 32


def fit_bands(H, W):
    """The smallest number of bands whose rows fit BAND_PIX pixels each."""
    return -(-H // (BAND_PIX // W))


def bands(B, H, W):
    """cloud_bands: bands per instance - enough for the parallelism of a small batch (8192 workgroups over the batch, at most 64 per
    instance, no band below four rows for parallelism's sake), and never fewer than BAND_PIX asks for."""
    if B <= 0 or H <= 0 or W <= 0 or W > BAND_PIX:
        return 0
    par = min(-(-WANT_WGS // B), MAX_BANDS, (H + 3) // 4)
    return max(fit_bands(H, W), par)


def scan_chunk(B):
    """Instances per thread of cloud_scan_kernel."""
    return -(-B // SCAN_THREADS)


def band_rows(nb, H):
    """The rows [v0, v1) of the non-empty bands of an instance of H rows split into nb bands (band_rows of la3d_cloud.hip)."""
    rpb = -(-H // nb)
    return [(b * rpb, min(H, (b + 1) * rpb)) for b in range(nb) if b * rpb < H]


def band_words(B, H, W):
    """64-pixel words of every non-empty band of a uniform call."""
    return [((v1 - v0) * W + 63) // 64 for v0, v1 in band_rows(bands(B, H, W), H)]


def u8_forms(B, H, W, n):
    """The forms band_bits takes for the bands of instance n of a dense, 16-byte aligned (B,H,W) u8 stack: "16" (16 pixels per thread
    and step: the band starts on a 16-byte address and holds a multiple of 16 pixels) or "general" (one ballot per word)."""
    return ["16" if (n * H * W + v0 * W) % 16 == 0 and ((v1 - v0) * W) % 16 == 0 else "general" for v0, v1 in band_rows(bands(B, H, W), H)]


# ------------------------------------------------------------------------------------------------------------------------------
# 16-bit depth: the value rule of include/la3d.h, restated (tests/depth16_cases.py holds the suite's copy; a CPU test compares them)
# ------------------------------------------------------------------------------------------------------------------------------
def quantise(d32, dtype, scale=0.001):
    d32 = np.asarray(d32, np.float32)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return d32.astype(np.float16)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = np.rint(d32 / np.float32(scale))
        q = np.where(np.isfinite(d32) & (d32 > 0), np.minimum(q, np.float32(65535)), np.float32(0))
    return q.astype(np.uint16)


def upconvert(x, scale=1.0, hole=True):
    x = np.asarray(x)
    if x.dtype == np.float16:
        return x.astype(np.float32)
    assert x.dtype == np.uint16
    v = x.astype(np.float32) * np.float32(scale)
    return np.where((x == 0) & bool(hole), np.float32("nan"), v).astype(np.float32)


def stored_planes(c, kind):
    """The 16-bit planes of a depth kind ("f16", "u16h", "u16n"), one per image."""
    return [quantise(d, "f16" if kind == "f16" else "u16", c["scale"]) for d in c["depth"]]


def value_planes(c, kind):
    """The float32 planes a run of this depth kind fits."""
    if kind == "f32":
        return c["depth"]
    return [upconvert(s, c["scale"], kind == "u16h") for s in stored_planes(c, kind)]


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
MASK_NAMES = ("empty", "first pixel", "last pixel", "full", "row", "column", "checkerboard", "random 2 %", "runs over 31|32 and 63|64",
              "blob > 64", "density", "one per 4096", "last pixel of a band", "first pixel of a band", "run across a band's first row",
              "runs across 64-pixel words", "exactly 500", "exactly 501")


def standard_masks(H, W, seed=0):
    """The ten masks every frame of tests/test_gpu_instance_points.py is tested with (tests/instance_points_cases.py; a CPU test
    compares the two)."""
    rs = np.random.RandomState(seed)
    m = np.zeros((10, H, W), bool)
    m[1, 0, 0] = True
    m[2, H - 1, W - 1] = True
    m[3] = True
    m[4, H // 2] = True
    m[5, :, W // 3] = True
    vv, uu = np.mgrid[0:H, 0:W]
    m[6] = (vv + uu) % 2 == 0
    m[7] = rs.rand(H, W) < 0.02
    m[7, rs.randint(0, H), W - 1] = m[7, rs.randint(0, H), max(W - 2, 0)] = m[7, rs.randint(0, H), max(W - 3, 0)] = True   # (max: frames below 3 columns)
    flat = m[8].reshape(-1)
    flat[28:36] = True; flat[60:68] = True
    if W > 68:
        m[8, H // 2, 28:36] = True; m[8, H // 2, 60:68] = True
        m[8, H - 1, 30:34] = True
    flat = m[9].reshape(-1)
    start = max(0, min(W + 3, H * W - 100))
    flat[start:min(H * W, start + 100)] = True
    return m


def special_plane(rs, H, W):
    """A float32 plane of 0.5 .. 10 m with NaN, +inf, 0, a negative depth and -inf sprinkled in (about one pixel in 400 each)."""
    d = rs.uniform(0.5, 10.0, (H, W)).astype(np.float32)
    f = d.reshape(-1)
    for val in (np.nan, np.inf, 0.0, -1.25, -np.inf):
        f[rs.randint(0, f.size, max(1, f.size // 400))] = val
    return d


def one_mask(rs, H, W, rows, std, capacity_frame, want_sample):
    """One mask of an H x W image whose instance is split into the bands `rows` -> (mask, kind: index into MASK_NAMES)."""
    n = H * W
    m = np.zeros(n, bool)
    u = rs.rand()
    if capacity_frame and u < 0.35:                      # (fewer of the standard masks there: the full one and the aimed ones are the point)
        if rs.rand() < 0.4:
            return std[3].copy(), 3
        u = 0.40 + 0.6 * rs.rand()
    if want_sample and n >= 501 and u < 0.12:
        k = 16 + rs.randint(0, 2)
        m[rs.choice(n, 500 + (k - 16), replace=False)] = True
    elif u < 0.40:
        k = rs.randint(0, 10)
        m = std[k].reshape(-1).copy()
    elif u < 0.55:
        if capacity_frame and rs.rand() < 0.5:
            k = 11                                           # one pixel in every run of 4096
            base = np.arange(0, n, 4096)
            m[np.minimum(base + rs.randint(0, 4096, len(base)), n - 1)] = True
        else:
            k = 10
            m = rs.rand(n) < 2.0 ** -rs.uniform(0, 16)
    elif u < 0.85:
        k = 12 + rs.randint(0, 3)
        for b in rs.choice(len(rows), min(len(rows), rs.randint(1, 4)), replace=False):
            v0, v1 = rows[b]
            if k == 12:
                m[v1 * W - 1] = True
            elif k == 13:
                m[v0 * W] = True
            else:
                m[max(0, v0 * W - rs.randint(1, 70)):min(n, v0 * W + rs.randint(1, 70))] = True
    else:
        k = 15
        for j in rs.randint(0, n // 64 + 1, rs.randint(1, 5)):
            m[max(0, 64 * j - rs.randint(1, 40)):min(n, 64 * j + rs.randint(1, 40))] = True
    return m.reshape(H, W), k


def draw_frames(rs):
    """-> (sizes of the P images, B, uniform, class of the case)."""
    if rs.rand() < 0.6:
        u = rs.rand()
        if u < 0.30:
            return [CAPACITY[rs.randint(len(CAPACITY))]], int(rs.randint(1, 4)), True, "capacity"
        if u < 0.36:
            return [BIG], int(rs.randint(1, 4)), True, "big"
        if u < 0.52:
            if rs.rand() < 0.15:
                return [(33, 47)], 2049, True, "large batch"
            return [SMALL[rs.randint(len(SMALL))]], LARGE_BS[rs.randint(len(LARGE_BS))], True, "large batch"
        return [TINY[rs.randint(len(TINY))]], BS[rs.randint(len(BS))], True, "tiny"
    P = int(rs.randint(4, 7))
    sizes = [TINY[i] for i in rs.choice(len(TINY), P, replace=False)]
    u = rs.rand()
    if u < 0.2:
        sizes[rs.randint(P)] = CAPACITY[rs.randint(len(CAPACITY))]
        return sizes, int(rs.randint(2, 4)), False, "capacity"
    if u < 0.3:
        sizes[rs.randint(P)] = BIG
        return sizes, int(rs.randint(2, 4)), False, "big"
    return sizes, [2, 3, 7, 33, 300][rs.randint(5)], False, "tiny"


def make_case(seed):
    """One case of the campaign (inputs only), deterministic from the seed."""
    rs = np.random.RandomState(seed)
    sizes, B, uniform, fclass = draw_frames(rs)
    if uniform:
        H, W = sizes[0]
        mode = rs.randint(0, 3)                            # 0: one shared plane, 1: private planes, 2: P planes + image_index
        if mode == 1 and (B > 33 or fclass in ("capacity", "big")):
            mode = 2
        P = 1 if mode == 0 else (B if mode == 1 else int(rs.randint(1, min(B, 5) + 1)))
        sizes = [(H, W)] * P
        img = np.zeros(B, np.int32) if mode == 0 else (np.arange(B, dtype=np.int32) if mode == 1 else rs.randint(0, P, B).astype(np.int32))
        ii_given = mode == 2
        none = None
    else:
        P = len(sizes)
        none = int(rs.randint(P))                          # the image without an instance
        img = rs.choice([p for p in range(P) if p != none], B).astype(np.int32)
        ii_given = True
    depth = [special_plane(rs, h, w) for h, w in sizes]
    skew = rs.rand() < 1 / 3
    K = np.zeros((P, 3, 3))
    for p, (h, w) in enumerate(sizes):
        # focal lengths proportional to W as in the hand-made tests - to H on a frame taller than wide (1000x1): a principal point
        # hundreds of focal lengths off the axis cancels in v - cy, and the oracle's own rounding then passes the 1e-13 it is the
        # yardstick of (test_cloud_slice_covers holds the oracle to a tenth of it on every case)
        f = max(h, w)
        K[p] = [[(0.8 + 0.4 * rs.rand()) * f, rs.uniform(-3, 3) if skew else 0.0, w / 2.0 + rs.uniform(-0.25, 0.25) * w],
                [0.0, (0.8 + 0.4 * rs.rand()) * f, h / 2.0 + rs.uniform(-0.25, 0.25) * h], [0.0, 0.0, 1.0]]
    k_shared = rs.rand() < 0.3
    if k_shared:
        K[:] = K[0]
    want_sample = rs.rand() < 0.4
    # the band split the masks aim at: the call's own (uniform: at the frame's width or its padded width; mixed: the frames call's,
    # whose band count comes from the largest rows and the largest pitch)
    Hc, Wc = max(h for h, _ in sizes), max(padded_width(w) for _, w in sizes)
    std, masks, mkind = {}, [], []
    for n in range(B):
        h, w = sizes[img[n]]
        if (h, w) not in std:
            std[(h, w)] = standard_masks(h, w, seed % 7)
        nb = bands(B, Hc, Wc) if not uniform else bands(B, h, w if rs.rand() < 0.5 else padded_width(w))
        m, k = one_mask(rs, h, w, band_rows(max(nb, 1), h), std[(h, w)], (h, w) in CAPACITY, want_sample)
        masks.append(m); mkind.append(k)
    bytes_kind = rs.randint(0, 3)
    vals = np.array([1, 2, 0x80, 0xff], np.uint8)
    mb = [np.where(m, 1 if bytes_kind == 0 else (255 if bytes_kind == 1 else vals[rs.randint(0, 4, m.shape)]), 0).astype(np.uint8) for m in masks]
    counts = np.array([int(m.sum()) for m in masks], np.int64)
    sidx = None
    if want_sample:
        sidx = np.zeros((B, NSAMPLE), np.int32)
        for n, cnt in enumerate(counts):
            if cnt > NSAMPLE:
                sidx[n] = rs.randint(0, int(cnt), NSAMPLE)
                v = rs.rand()
                if v < 0.25:
                    sidx[n, 10:13] = sidx[n, 10]                                 # repeated ranks
                elif v < 0.5:
                    sidx[n, 0], sidx[n, 1], sidx[n, 499] = cnt, -1, cnt - 1      # outside the cloud, and the last rank
                elif v < 0.6:
                    sidx[n, rs.randint(0, NSAMPLE, 40)] = rs.choice([-1, cnt, cnt + 7, -2 ** 31, 2 ** 31 - 1], 40)
            elif rs.rand() < 0.3:
                sidx[n] = rs.choice([-1, 0, cnt, 2 ** 31 - 1, 77], NSAMPLE)      # the rule never looks at this row
    rows = np.where((counts > NSAMPLE) & (sidx is not None), NSAMPLE, counts)
    off = np.concatenate([[0], np.cumsum(rows)])
    cap = None
    if rows.any():
        n = int(rs.choice(np.flatnonzero(rows)))
        cap = int(off[n] + rs.randint(0, rows[n]))         # inside instance n's range: it and everything behind it must not fit
    H0, W0 = sizes[0]
    v = rs.rand()
    cfw = 1 if v < 0.12 else (W0 if v < 0.22 else (int(rs.randint(1, W0 - 64)) if v < 0.6 and W0 > 66 else int(rs.randint(1, W0 + 1))))
    return dict(seed=seed, P=P, B=B, sizes=sizes, uniform=uniform, fclass=fclass, H=H0 if uniform else None, W=W0 if uniform else None,
                img=img, image_index=img if ii_given else None, none=none, depth=depth, K=K, k_shared=k_shared, skew=skew, masks=masks,
                mb=mb, mkind=mkind, bytes_kind=bytes_kind, counts=counts, sidx=sidx, cap=cap, perm=rs.permutation(B),
                frames16=DEPTH_KINDS[1 + rs.randint(0, 3)], scale=SCALES[rs.randint(len(SCALES))], cfw=cfw, cbase=int(1 + 2 * rs.randint(0, 8)),
                cextra=int(rs.randint(1, 41)))


def features(c):
    """What a case brings to a slice, from the generator alone -> set of names (tests/test_differential_checkers.py::
    test_cloud_slice_covers lists the ones a slice must hold)."""
    f = set()
    B, counts = c["B"], c["counts"]
    f.add(f"scan chunk {scan_chunk(B)}")
    f.add(f"B = {B}")
    f.add("skew" if c["skew"] else "no skew")
    f.add(f"u8 bytes {c['bytes_kind']}")
    nz = np.flatnonzero(counts)
    if not len(nz):
        f.add("all empty")
    else:
        if counts[0] == 0:
            f.add("empty first")
        if counts[-1] == 0:
            f.add("empty last")
        if (counts[nz[0]:nz[-1]] == 0).any():
            f.add("empty between")
    if c["k_shared"] and c["P"] > 1 and c["image_index"] is not None:
        f.add("K shared, P > 1, image_index")
    if not c["uniform"] and len(set(c["sizes"])) >= 4 and not (c["img"] == c["none"]).any():
        f.add("mixed: four sizes, one without an instance")
    # bands: of the uniform u8 / bit-plane call (pitch W) and of the frames call (padded pitch, band count from the call's bounds)
    Hc, Wc = max(h for h, _ in c["sizes"]), max(padded_width(w) for _, w in c["sizes"])
    for n in range(B):
        h, w = c["sizes"][c["img"][n]]
        forms = [("frames", bands(B, Hc, Wc), padded_width(w))] + ([("uniform", bands(B, h, w), w)] if c["uniform"] else [])
        for form, nb, pitch in forms:
            for v0, v1 in band_rows(nb, h):
                words = ((v1 - v0) * pitch + 63) // 64
                if words < 1024:
                    continue
                f.add(f"{form}: band of 1024 words")
                rows = c["masks"][n][v0:v1]
                cnt = int(rows.sum())
                if cnt == BAND_PIX:
                    f.add(f"{form}: band of 1024 words, all 65536 pixels set")
                if (v1 - v0) * pitch == BAND_PIX - 1:
                    f.add(f"{form}: band of 1024 words, the last one short")
                if pitch > w:
                    f.add("frames: rows padded to a pitch of 65536")
                if 0 < cnt < 32:
                    at = np.flatnonzero(np.pad(rows, ((0, 0), (0, pitch - w))).reshape(-1)) // 64
                    if at[-1] - at[0] > 512:
                        f.add(f"{form}: capacity band with fewer than 32 pixels over more than 512 words")
        if c["uniform"]:
            if fit_bands(h, w) > min(-(-WANT_WGS // B), MAX_BANDS, (h + 3) // 4):
                f.add("band count from BAND_PIX")
            if fit_bands(h, w) < bands(B, h, w) and len(band_rows(bands(B, h, w), h)) < bands(B, h, w):
                f.add("trailing empty bands")
            if counts[n] and len(set(u8_forms(B, h, w, n))) == 2:
                f.add("u8: both forms in one instance")
    if c["uniform"]:
        if c["W"] - c["cfw"] > 64:
            f.add("C entry: more than 64 padding columns")
        if c["cfw"] == 1:
            f.add("C entry: frame_width 1")
    if c["sidx"] is not None:
        big = np.flatnonzero(counts > NSAMPLE)
        if 16 in c["mkind"]:
            f.add("subsample: exactly 500 pixels")
        if 17 in c["mkind"]:
            f.add("subsample: exactly 501 pixels")
        for n in big:
            r = c["sidx"][n].astype(np.int64)
            if ((r < 0) | (r >= counts[n])).any():
                f.add("subsample: ranks outside the cloud")
            if len(np.unique(r)) < NSAMPLE:
                f.add("subsample: repeated ranks")
            if (r == counts[n] - 1).any():
                f.add("subsample: the last rank")
        if len(big):
            for r in RUNS:
                if applies(c, r) and r:
                    f.add(f"subsample: {r}")
    return f


# ------------------------------------------------------------------------------------------------------------------------------
# oracle
# ------------------------------------------------------------------------------------------------------------------------------
def instance_rows(cloud, flat, W, fw, ranks):
    """The rows of one instance: `cloud` (H*W, 3) the plane's points, `flat` its mask - row-major order is the order of the flat
    pixel index -, columns >= fw are no pixels, a pixel is reported as v * fw + u; `ranks`: the instance's sample_idx row or None.
    -> (points, pixels, count)."""
    idx = np.flatnonzero(flat)
    v, u = idx // W, idx % W
    keep = u < fw
    idx, pix = idx[keep], (v[keep] * fw + u[keep]).astype(np.int32)
    N = len(idx)
    if ranks is None or N <= NSAMPLE:
        return cloud[idx], pix, N
    r = np.asarray(ranks, np.int64)
    inside = (r >= 0) & (r < N)
    pts, px = np.full((NSAMPLE, 3), np.nan), np.full(NSAMPLE, -1, np.int32)
    pts[inside], px[inside] = cloud[idx[r[inside]]], pix[r[inside]]
    return pts, px, N


def expected(c):
    """The oracle's result of a case for every variant a run can ask for -> {variant: dict(points, pixels: lists over the instances;
    counts (B,); fw: the frame width the pixels count in, per instance), "clouds": {depth kind: the points of every plane (H*W, 3)}}.
    Variants: the depth kinds of DEPTH_KINDS and - uniform cases - "c_u8": float32 planes with the frame_width of the C-entry run."""
    from oracle import la3d_oracle as O

    out, clouds = {}, {}
    for kind in DEPTH_KINDS:
        planes = value_planes(c, kind)
        clouds[kind] = [O.depth_to_points(planes[p][None], c["K"][p]).reshape(-1, 3) for p in range(c["P"])]
    variants = [(k, None) for k in DEPTH_KINDS] + ([("c_u8", c["cfw"])] if c["uniform"] else [])
    for name, fw in variants:
        kind = "f32" if name == "c_u8" else name
        pts, pix, counts = [], [], np.zeros(c["B"], np.int32)
        for n in range(c["B"]):
            p = int(c["img"][n])
            W = c["sizes"][p][1]
            a, b, counts[n] = instance_rows(clouds[kind][p], c["masks"][n].reshape(-1), W, W if fw is None else fw,
                                            None if c["sidx"] is None else c["sidx"][n])
            pts.append(a); pix.append(b)
        out[name] = dict(points=pts, pixels=pix, counts=counts, fw=fw)
    out["clouds"] = clouds
    return out


_WANT = {}


def oracle_case(seed):
    """expected(make_case(seed)), kept for the process (the CPU tests and the GPU slice share it)."""
    if seed not in _WANT:
        _WANT[seed] = expected(make_case(seed))
    return _WANT[seed]


def packed(want, order):
    """The instances of one variant in the order of a run -> (points (T,3), pixels (T,), offsets (B+1,), counts (B,))."""
    pts = [want["points"][n] for n in order]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64)
    return (np.concatenate(pts) if len(pts) else np.zeros((0, 3)), np.concatenate([want["pixels"][n] for n in order]) if len(pts) else
            np.zeros(0, np.int32), off, want["counts"][order])


def longdouble_cloud(plane, K):
    """The formula of depth_to_points in np.longdouble with K inverted in closed form: what the oracle's own rounding is measured
    against (tests/test_differential_checkers.py::test_cloud_slice_covers)."""
    L = np.longdouble
    fx, s, cx, fy, cy = (L(K[0, 0]), L(K[0, 1]), L(K[0, 2]), L(K[1, 1]), L(K[1, 2]))
    assert K[1, 0] == 0 and K[2, 0] == 0 and K[2, 1] == 0 and K[2, 2] == 1
    H, W = plane.shape
    d = plane.astype(L)
    u, v = np.arange(W, dtype=L)[None, :], np.arange(H, dtype=L)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        y = (v - cy) / fy
        x = (u - cx - s * y) / fx
        return np.stack([d * x, d * y, d * np.ones((H, W), L)], -1).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU runs
# ------------------------------------------------------------------------------------------------------------------------------
RUNS = [dict(),                                  # u8 planes, float64, pixels: the default run
        dict(entry="bits", frame_pad=True), dict(entry="bits", frame_pad=False),
        dict(out="f32"),
        dict(depth="f16"), dict(depth="u16h"), dict(depth="u16n"),
        dict(entry="frames"), dict(entry="frames", depth="16"),   # (the 16-bit kind of a frames run: the case's frames16)
        dict(capacity="short"),
        dict(entry="c_u8")]                      # the C entry on u8 planes in place: plane stride, odd base, frame_width from [1, W]


def applies(c, r):
    """The frames runs take every case; everything else needs images of one size; a short capacity needs a row to cut."""
    if r.get("entry") == "frames":
        return True
    if not c["uniform"]:
        return False
    return c["cap"] is not None if r.get("capacity") else True


def variant(c, r):
    """(variant of expected(c) the run is held to, depth kind of the planes it reads)"""
    if r.get("entry") == "c_u8":
        return "c_u8", "f32"
    k = r.get("depth", "f32")
    k = c["frames16"] if k == "16" else k
    return k, k


def run_order(c, r):
    """row of the run -> instance of the case: the frames runs list the instances image by image and then permute them"""
    if r.get("entry") != "frames":
        return np.arange(c["B"])
    return np.argsort(c["img"], kind="stable")[c["perm"]]


def run_gpu(c, r, cache=None):
    """One run of a case on the GPU -> dict of NumPy arrays: points, pixels (None: not asked for), offsets, counts, status, order
    (run_order), rows (per image the (H*W, 3) rows of la.unproject of the planes the run read), capacity (the short-capacity run:
    its buffers are longer than that and were filled with SENT).  Raises what the call raises."""
    import ctypes as C

    import torch

    import labelany3d_amd as la
    from labelany3d_amd import _lib

    cache = {} if cache is None else cache
    np_ = lambda t: t.detach().cpu().numpy()   # noqa: E731
    dev = "cuda"
    name, kind = variant(c, r)
    entry, B, P = r.get("entry"), c["B"], c["P"]
    order = run_order(c, r)
    K = c["K"][0] if c["k_shared"] else c["K"]
    hole = kind == "u16h"

    def stored():
        if ("stored", kind) not in cache:
            cache[("stored", kind)] = stored_planes(c, kind)
        return cache[("stored", kind)]

    if ("rows", kind) not in cache:
        rows = []
        for p in range(P):
            if kind == "f32":
                plane = torch.as_tensor(c["depth"][p], device=dev)
            else:
                plane = la.unpack_depth16(la.Depth16(torch.as_tensor(stored()[p], device=dev), c["scale"], hole))
            rows.append(np_(la.unproject(plane[None], c["K"][p][None])).reshape(-1, 3))
        cache[("rows", kind)] = rows
    got = dict(order=order, rows=cache[("rows", kind)], capacity=None)
    sidx = c["sidx"]

    if entry == "frames":
        if "fb" not in cache:
            stacks = [np.stack([c["mb"][n] for n in np.flatnonzero(c["img"] == p)]) if (c["img"] == p).any() else np.zeros((0,) + c["sizes"][p], np.uint8)
                      for p in range(P)]
            fb = la.pack_mask_bits_frames(la.pack_mask_frames(stacks))
            t = torch.as_tensor(c["perm"], device=dev)
            cache["fb"] = fb._replace(offsets=fb.offsets[t].contiguous(), image_index=fb.image_index[t].contiguous(), area=fb.area[t].contiguous())
        if kind == "f32":
            pf = la.pack_frames(c["depth"])
        else:
            pf = la.pack_frames(stored(), dtype="f16" if kind == "f16" else "u16", scale=c["scale"], zero_is_hole=hole)
        ip = la.instance_points_frames(pf, cache["fb"], K, sample_idx=None if sidx is None else sidx[order], pixels=True)
    elif entry == "c_u8":
        H, W, fw = c["H"], c["W"], c["cfw"]
        stride, base = H * W + c["cextra"], c["cbase"]
        host = np.zeros(base + B * stride, np.uint8)
        for n in range(B):
            host[base + n * stride:base + n * stride + H * W] = c["mb"][n].reshape(-1)
        buf = torch.as_tensor(host, device=dev)
        d, k = torch.as_tensor(np.stack(c["depth"]), device=dev), torch.as_tensor(np.ascontiguousarray(K), device=dev)   # (one matrix, or P)
        ii = None if c["image_index"] is None else torch.as_tensor(c["image_index"], device=dev)
        si = None if sidx is None else torch.as_tensor(sidx, device=dev)
        ws = torch.empty(max(_lib.lib.la3d_instance_points_workspace_bytes(B, H, W) // 4, 1), dtype=torch.int32, device=dev)
        counts, offsets = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B + 1, dtype=torch.int64, device=dev)
        a = _lib.CloudArgs(struct_size=C.sizeof(_lib.CloudArgs), B=B, H=H, W=W, frame_width=fw, depth=d.data_ptr(),
                           depth_plane_stride=H * W if P > 1 else 0, mask=buf.data_ptr() + base, mask_plane_stride=stride, K=k.data_ptr(),
                           k_stride=0 if c["k_shared"] or P == 1 else 9, image_index=None if ii is None else ii.data_ptr(),
                           sample_idx=None if si is None else si.data_ptr(), counts=counts.data_ptr(), offsets=offsets.data_ptr(),
                           workspace=ws.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib.la3d_instance_point_offsets(C.byref(a)), "la3d_instance_point_offsets")
        cap = int(offsets[-1].item())
        pts, pix = torch.empty((cap, 3), dtype=torch.float64, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        a.points, a.pixels, a.status, a.capacity, a.out_is_f64 = pts.data_ptr(), pix.data_ptr(), status.data_ptr(), cap, 1
        _lib.check(_lib.lib.la3d_gather_instance_points(C.byref(a)), "la3d_gather_instance_points")
        torch.cuda.synchronize()
        ip = la.InstancePoints(pts, offsets, counts, pix, status)
    else:
        if "mb" not in cache:
            cache["mb"] = torch.as_tensor(np.stack(c["mb"]), device=dev)
        masks = cache["mb"]
        if entry == "bits":
            masks = la.pack_mask_bits(masks, frame_pad=r["frame_pad"])
        if kind == "f32":
            depth = np.stack(c["depth"])
        else:
            depth = la.Depth16(torch.as_tensor(np.stack(stored()), device=dev), c["scale"], hole)
        kw = dict(image_index=c["image_index"], sample_idx=sidx)
        if r.get("capacity"):
            total = int(np.where((c["counts"] > NSAMPLE) & (sidx is not None), NSAMPLE, c["counts"]).sum())
            out = (torch.full((total + 64, 3), SENT, dtype=torch.float64, device=dev), torch.full((total + 64,), int(SENT), dtype=torch.int32, device=dev),
                   torch.full((B,), -9, dtype=torch.int32, device=dev))
            ip = la.instance_points(depth, masks, K, capacity=c["cap"], pixels=True, _out=out, **kw)
            got["capacity"] = c["cap"]
        elif r.get("out") == "f32":
            ip = la.instance_points(depth, masks, K, out_dtype=torch.float32, **kw)
        else:
            ip = la.instance_points(depth, masks, K, pixels=True, **kw)
    got.update(points=np_(ip.points), pixels=None if ip.pixels is None else np_(ip.pixels), offsets=np_(ip.offsets), counts=np_(ip.counts),
               status=np_(ip.status))
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# the checker
# ------------------------------------------------------------------------------------------------------------------------------
RULES = ("counts", "offsets", "status", "shape", "pixels", "rows", "oracle", "cast", "default", "sentinel")


def _same(a, b):
    """row-wise equality, NaN equal to NaN"""
    a, b = np.asarray(a), np.asarray(b)
    eq = (a == b) | ((a != a) & (b != b))
    return eq.all(axis=1)


def _inst(off, rows):
    """the instances (rows of the run) that hold the given output rows"""
    return sorted(set((np.searchsorted(off, rows, side="right") - 1).tolist()))


def check_run(c, want, r, got, default=None, rules=RULES):
    """Compare one run's GPU output (run_gpu's dict) with want = expected(c).  `default`: the default run's output of the same case
    (uniform cases) for the comparisons between runs.  Returns the failures as strings, each naming run rows / instances and the
    field (empty: the run agrees).  `rules`: the rules to apply - all of them; the CPU test of the checker takes them out one by
    one."""
    name, kind = variant(c, r)
    w = want[name]
    order, B = got["order"], c["B"]
    pts_w, pix_w, off_w, cnt_w = packed(w, order)
    inst = lambda rows: [f"{i} (instance {int(order[i])}, mask '{MASK_NAMES[c['mkind'][order[i]]]}')" for i in rows[:4]]   # noqa: E731
    fails = []
    cap = got["capacity"]
    st_w = np.zeros(B, np.int32) if cap is None else (off_w[1:] > cap).astype(np.int32)
    pts, pix, off, cnt, st = got["points"], got["pixels"], got["offsets"], got["counts"], got["status"]
    if "counts" in rules and (cnt.shape != cnt_w.shape or (cnt != cnt_w).any()):
        bad = np.flatnonzero(cnt != cnt_w) if cnt.shape == cnt_w.shape else []
        fails.append(f"counts differ at rows {inst(bad)}: got {cnt[bad][:4].tolist() if len(bad) else cnt.shape} expected {cnt_w[bad][:4].tolist()}")
    if "offsets" in rules and (off.shape != off_w.shape or (off != off_w).any()):
        bad = np.flatnonzero(off != off_w) if off.shape == off_w.shape else []
        fails.append(f"offsets differ at {bad[:4].tolist() if len(bad) else off.shape}: got {off[bad][:4].tolist() if len(bad) else ''} expected {off_w[bad][:4].tolist()}")
    if "status" in rules and (st.shape != st_w.shape or (st != st_w).any()):
        bad = np.flatnonzero(st != st_w) if st.shape == st_w.shape else []
        fails.append(f"status differs at rows {inst(bad)}: got {st[bad][:4].tolist() if len(bad) else st.shape} expected {st_w[bad][:4].tolist()}"
                     + ("" if cap is None else f" (capacity {cap}, offsets {off_w[bad][:4].tolist()} .. {off_w[1:][bad][:4].tolist()})"))
    T = int(off_w[-1])
    f32 = r.get("out") == "f32"
    room = T if cap is None else T + 64
    if "shape" in rules:
        if pts.shape != (room, 3) or pts.dtype != (np.float32 if f32 else np.float64):
            fails.append(f"points: shape {pts.shape} dtype {pts.dtype}, expected {(room, 3)}")
        if (pix is None) != f32 or (pix is not None and (pix.shape != (room,) or pix.dtype != np.int32)):
            fails.append(f"pixels: {None if pix is None else (pix.shape, pix.dtype)}, expected {None if f32 else (room,)}")
    if pts.shape[0] < T or (pix is not None and pix.shape[0] < T):
        return fails + ["the output holds fewer rows than the oracle's offsets[-1]: no row compared"]
    live = np.repeat(st_w == 0, np.diff(off_w))                        # rows of the instances that must have been written
    rows_live = np.flatnonzero(live)
    # the rows the clouds are cut from: la.unproject of the planes the run read, at the pixel the oracle expects (v * W + u)
    W_of = np.array([c["sizes"][p][1] for p in c["img"][order]], np.int64)
    fw_of = W_of if w["fw"] is None else np.full(B, w["fw"], np.int64)
    Wr, fwr = np.repeat(W_of, np.diff(off_w)), np.repeat(fw_of, np.diff(off_w))
    img_r = np.repeat(c["img"][order], np.diff(off_w))
    if "pixels" in rules and pix is not None:
        bad = rows_live[pix[:T][live] != pix_w[live]]
        if len(bad):
            fails.append(f"pixels differ in {len(bad)} rows of run rows {inst(_inst(off_w, bad))}: row {bad[0]} got {pix[bad[0]]} expected {pix_w[bad[0]]}")
    if "rows" in rules:
        cut = np.full((T, 3), np.nan)
        for p in range(c["P"]):
            sel = (img_r == p) & (pix_w >= 0)
            px = pix_w[sel].astype(np.int64)
            cut[sel] = got["rows"][p][(px // fwr[sel]) * Wr[sel] + px % fwr[sel]]
        cut = cut.astype(np.float32) if f32 else cut
        bad = rows_live[~_same(pts[:T][live], cut[live])]
        if len(bad):
            fails.append(f"points: {len(bad)} rows are not the unproject rows of their pixels, bit for bit, in run rows {inst(_inst(off_w, bad))}: "
                         f"row {bad[0]} (pixel {pix_w[bad[0]]}) got {pts[bad[0]].tolist()} expected {cut[bad[0]].tolist()}")
    if "oracle" in rules:
        ref = pts_w.astype(np.float32) if f32 else pts_w
        a, b = pts[:T][live].astype(np.float64), ref[live].astype(np.float64)
        with np.errstate(invalid="ignore"):
            # float32 output: one rounding of a value within TOL of the oracle's lies within one float32 step of the oracle's rounding
            tol = TOL + TOL * np.abs(b) + (np.abs(np.spacing(b.astype(np.float32)).astype(np.float64)) if f32 else 0.0)
            ok = (np.abs(a - b) <= tol) | (a == b) | ((a != a) & (b != b))
        bad = rows_live[~ok.all(1)]
        if len(bad):
            fails.append(f"points: {len(bad)} rows beyond rtol = atol = {TOL} of the oracle in run rows {inst(_inst(off_w, bad))}: row {bad[0]} got "
                         f"{pts[bad[0]].tolist()} expected {ref[bad[0]].tolist()}")
    if default is not None and (f32 or r.get("entry") in ("bits", "frames")) and kind == "f32":
        # between runs: the rows of the default run, instance by instance (a frames run lists them in another order)
        d_off = default["offsets"]
        src = np.concatenate([np.arange(d_off[n], d_off[n + 1]) for n in order]) if B else np.zeros(0, np.int64)
        if len(src) != T or default["points"].shape[0] < T:
            fails.append("the default run has other offsets: no comparison between the runs")
        elif f32 and "cast" in rules:
            bad = np.flatnonzero(~_same(pts[:T], default["points"][src].astype(np.float32)))
            if len(bad):
                fails.append(f"float32 points: {len(bad)} rows are not the cast of the float64 run's, in run rows {inst(_inst(off_w, bad))}")
        elif not f32 and "default" in rules:
            bad = np.flatnonzero(~_same(pts[:T], default["points"][src]) | (pix[:T] != default["pixels"][src]))
            if len(bad):
                fails.append(f"points / pixels: {len(bad)} rows differ from the default run's, in run rows {inst(_inst(off_w, bad))}")
    if "sentinel" in rules and cap is not None:
        dead = ~live
        bad = np.flatnonzero(dead & ~((pts[:T] == SENT).all(1) & (pix[:T] == int(SENT))))
        if len(bad):
            fails.append(f"points / pixels: {len(bad)} rows written inside the range of an instance beyond the capacity {cap}, run rows {inst(_inst(off_w, bad))}")
        if not ((pts[T:] == SENT).all() and (pix[T:] == int(SENT)).all()):
            fails.append(f"points / pixels: written at or beyond offsets[-1] = {T}")
    return fails


def new_tally():
    return dict(cases=0, instances=0, calls=0, rows=0, full_bands=0, chunks=set(), sampled=0)


def tally_case(t, c, want):
    t["cases"] += 1
    t["instances"] += c["B"]
    t["rows"] += int(sum(len(p) for p in want["f32"]["points"]))
    t["chunks"].add(scan_chunk(c["B"]))
    t["sampled"] += c["sidx"] is not None
    t["full_bands"] += any("band of 1024 words" in f for f in features(c))


def tally_lines(t):
    return [f"{t['cases']} cases, {t['instances']} instances, {t['rows']} rows of the float32 variant, {t['calls']} calls; {t['sampled']} cases in "
            f"subsample mode; {t['full_bands']} cases with bands of 1024 words; scan chunks {sorted(t['chunks'])}"]
