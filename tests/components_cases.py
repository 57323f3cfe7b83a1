"""Connected components on bit planes (include/la3d.h "connected components on bit planes"): the NumPy restatement of the rule and the
case lists the host and the GPU tests share.  ``label`` is written from the rule as the header states it - a union-find over PIXELS
(hooking to the smaller root over every pair of adjacent set pixels, then pointer jumping, until nothing moves), components numbered by
the raster order of their first pixel -, not from SciPy's text; tests/golden/g20_components.npz (make_golden_components.py) holds what
``scipy.ndimage.label`` itself gives on the fixture planes."""
import hashlib
import os

import numpy as np

from .open_bits_cases import blob_plane, pack, padded, unpack, words  # noqa: F401  (the helpers of the opening's cases)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_components.npz")
SMALL_FRAMES = ((1, 1), (1, 33), (33, 1), (33, 47), (96, 224), (140, 96))      # (H, W)
WIDTHS = (31, 32, 33, 63, 64, 65)
WIDTH_ROWS = 13
FIXTURE_FRAMES = ((33, 47), (96, 224), (140, 96))
FIXTURE_PLANES = 3                             # planes per fixture frame
BIG_FRAME = (480, 640)
BIG_SEEDS = (2002, 2003, 2009)
SEED = 20
TABLE_ROWS = 64                                # table rows the fixture stores per plane
MIN_AREA = 4                                   # the min_area rule of the fixture and of the cases that name none
RULES = ((0, False), (MIN_AREA, False), (0, True))     # (min_area, largest): all, min_area, largest
DENSITIES = (0.3, 0.41, 0.5, 0.59, 0.7, 0.9)   # 0.41: the site-percolation threshold at 8, 0.59: at 4
MAX_CASE_RUNS = 3500
SENTINEL = 0x5A5A5A5A


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def label(mask, connectivity=8):
    """(H, W) bool -> (labels int32 (H, W), n): 0 = background, components 1 .. n in raster order of their first pixel"""
    m = np.asarray(mask, bool)
    H, W = m.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    pairs = [(m[:, :-1] & m[:, 1:], idx[:, :-1], idx[:, 1:]), (m[:-1] & m[1:], idx[:-1], idx[1:])]
    if connectivity == 8:
        pairs += [(m[:-1, :-1] & m[1:, 1:], idx[:-1, :-1], idx[1:, 1:]), (m[:-1, 1:] & m[1:, :-1], idx[:-1, 1:], idx[1:, :-1])]
    a = np.concatenate([p[k] for k, p, q in pairs])
    b = np.concatenate([q[k] for k, p, q in pairs])
    parent = np.arange(H * W, dtype=np.int64)
    while True:
        pa, pb = parent[a], parent[b]
        if np.array_equal(pa, pb):
            break
        lo = np.minimum(pa, pb)
        np.minimum.at(parent, pa, lo)          # hook the roots (or what was a root a moment ago) to the smaller side
        np.minimum.at(parent, pb, lo)
        while True:                            # pointer jumping: every pixel points at its root
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    flat = m.reshape(-1)
    roots = np.flatnonzero(flat & (parent == np.arange(H * W)))           # ascending: raster order of the first pixel
    rank = np.zeros(H * W, np.int32)
    rank[roots] = np.arange(1, len(roots) + 1)
    return np.where(flat, rank[parent], 0).astype(np.int32).reshape(H, W), int(len(roots))


def rect(mask):
    """x, y, w, h: the tight box of the set pixels (cv2.boundingRect of a binary image), zeros for an empty mask"""
    m = np.asarray(mask, bool)
    if not m.any():
        return [0, 0, 0, 0]
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    return [int(cols[0]), int(rows[0]), int(cols[-1] - cols[0] + 1), int(rows[-1] - rows[0] + 1)]


def table_of(labels, n):
    """-> int32 (n, 5): area, x, y, w, h of label j + 1 in row j"""
    t = np.zeros((n, 5), np.int32)
    if n == 0:
        return t
    vv, uu = np.nonzero(labels)
    lab = labels[vv, uu] - 1
    t[:, 0] = np.bincount(lab, minlength=n)
    x0 = np.full(n, 1 << 30); y0 = np.full(n, 1 << 30); x1 = np.full(n, -1); y1 = np.full(n, -1)
    np.minimum.at(x0, lab, uu); np.minimum.at(y0, lab, vv); np.maximum.at(x1, lab, uu); np.maximum.at(y1, lab, vv)
    t[:, 1], t[:, 2], t[:, 3], t[:, 4] = x0, y0, x1 - x0 + 1, y1 - y0 + 1
    return t


def choose(labels, n, table, min_area=0, largest=False):
    """the rule of the entry on a labelling -> (out (H, W) bool, stats [8])"""
    areas = table[:, 0]
    kept = np.flatnonzero(areas >= min_area)
    if largest and len(kept):
        kept = kept[[int(np.argmax(areas[kept]))]]          # argmax: the first of the greatest - the lowest label
    keep = np.zeros(n + 1, bool)
    keep[kept + 1] = True
    out = keep[labels]
    return out, [n, int(len(kept)), int((labels > 0).sum()), int(out.sum()), *rect(out)]


def components(mask, connectivity=8, min_area=0, largest=False, max_components=0):
    """-> (out bool, stats int32 [8], table int32 (max_components, 5)): what la3d_components_bits gives for one plane"""
    labels, n = label(mask, connectivity)
    t = table_of(labels, n)
    out, stats = choose(labels, n, t, min_area, largest)
    tab = np.zeros((max_components, 5), np.int32)
    tab[:min(n, max_components)] = t[:max_components]
    return out, np.asarray(stats, np.int32), tab


def count_runs(mask):
    """maximal horizontal spans of set pixels within a row"""
    m = np.asarray(mask, bool)
    return int(m[:, 0].sum() + (m[:, 1:] & ~m[:, :-1]).sum())


def words_sha256(mask, W_out):
    return hashlib.sha256(words(mask, W_out).astype("<u4").tobytes()).hexdigest()


# ---- patterns ----------------------------------------------------------------------------------------------------------------------
def spiral(H, W):
    """one component, a line one pixel wide wound inwards with one pixel between the turns: long merges"""
    m = np.zeros((H, W), bool)
    t, l, b, r = 0, 0, H - 1, W - 1
    first = True
    while t <= b and l <= r:
        m[t, (l if first else max(l - 1, 0)):r + 1] = True           # along the top, joined to the turn before
        m[t:b + 1, r] = True
        if b > t:
            m[b, l:r + 1] = True
        if r > l and b > t + 2:
            m[t + 2:b + 1, l] = True
        t, l, b, r = t + 2, l + 2, b - 2, r - 2
        first = False
        if t <= b and l <= r:
            m[t, l - 1] = True                                         # the bridge from the left side to the next turn
    return m


def comb(H, W):
    """teeth on the even columns that meet only in the last row: every equivalence is found late"""
    m = np.zeros((H, W), bool)
    m[:, ::2] = True
    m[H - 1, :] = True
    return m


def checkerboard(H, W):
    vv, uu = np.mgrid[0:H, 0:W]
    return (vv + uu) % 2 == 0


def diagonals(H, W, period=4):
    """lines along both diagonals' direction v + u = const: one component each at 8, single pixels at 4"""
    vv, uu = np.mgrid[0:H, 0:W]
    return (vv + uu) % period == 0


def ring_with_dot(H, W):
    m = np.zeros((H, W), bool)
    if H < 5 or W < 5:
        m[H // 2, W // 2] = True
        return m
    m[0, :] = m[H - 1, :] = True
    m[:, 0] = m[:, W - 1] = True
    m[H // 2, W // 2] = True
    return m


def seams(H, W):
    """pixels on either side of the word boundary 31|32 (one run), and the last column of a row with the first of the next (never joined)"""
    m = np.zeros((H, W), bool)
    for v in range(0, H - 1, 3):
        m[v, W - 1] = True
        m[v + 1, 0] = True
    if W > 32 and H > 2:
        m[H - 1, 31] = m[H - 1, 32] = True
    return m


def equal_pair(H, W):
    """two components of equal area: largest keeps the one whose first pixel comes first"""
    m = np.zeros((H, W), bool)
    h, w = max(1, H // 3), max(1, (W - 1) // 2)
    m[H - h:, :w] = True                       # lower left: its first pixel comes later
    m[:h, W - w:] = True                       # upper right
    return m


def area_steps(H, W, min_area=MIN_AREA):
    """horizontal bars of min_area - 1, min_area and min_area + 1 pixels, two rows apart"""
    m = np.zeros((H, W), bool)
    for i, n in enumerate((min_area - 1, min_area, min_area + 1, min_area, min_area - 1)):
        if 2 * i < H:
            m[2 * i, :min(n, W)] = True
    return m


PATTERNS = (("spiral", spiral), ("comb", comb), ("checkerboard", checkerboard), ("diagonals", diagonals), ("ring", ring_with_dot),
            ("seams", seams), ("equal_pair", equal_pair), ("area_steps", area_steps),
            ("empty", lambda H, W: np.zeros((H, W), bool)), ("full", lambda H, W: np.ones((H, W), bool)))


def frames():
    return list(SMALL_FRAMES) + [(WIDTH_ROWS, w) for w in WIDTHS]


def pattern_cases():
    """-> list of (name, mask): every pattern on every frame, with at most MAX_CASE_RUNS runs each - a pattern too dense for a frame
    (checkerboard, comb, spiral, diagonals on the two largest) fills only the frame's lower right 60 x 100 corner, the last row and
    the last column included"""
    out = []
    for H, W in frames():
        for name, fn in PATTERNS:
            m = fn(H, W)
            if count_runs(m) > MAX_CASE_RUNS:
                h, w = min(H, 60), min(W, 100)
                m = np.zeros((H, W), bool)
                m[H - h:, W - w:] = fn(h, w)
            assert count_runs(m) <= MAX_CASE_RUNS, (name, H, W)
            out.append((f"{name}_{H}x{W}", m))
    return out


def random_cases(seed=SEED, per_density=4):
    """-> list of (name, mask): H <= 70, W <= 100, every density of DENSITIES"""
    rs = np.random.RandomState(seed)
    out = []
    for d in DENSITIES:
        for i in range(per_density):
            H, W = rs.randint(1, 71), rs.randint(1, 101)
            out.append((f"random_{d}_{i}_{H}x{W}", rs.rand(H, W) < d))
    return out


def all_cases():
    return pattern_cases() + random_cases()


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def fixture_planes():
    """-> list, per fixture frame, of the (FIXTURE_PLANES, H, W) bool inputs"""
    rs = np.random.RandomState(SEED)
    return [np.stack([blob_plane(rs, H, W) for _ in range(FIXTURE_PLANES)]) for H, W in FIXTURE_FRAMES]


def big_planes():
    """-> (3, 480, 640) bool: blobs with 2 % salt noise, 6.2 - 6.6 k runs each"""
    return np.stack([blob_plane(np.random.RandomState(s), *BIG_FRAME) for s in BIG_SEEDS])


def fixture_keys():
    """-> list of (key, frame index or -1 for the big planes, plane, connectivity, min_area, largest)"""
    out = []
    for f in list(range(len(FIXTURE_FRAMES))) + [-1]:
        for p in range(FIXTURE_PLANES if f >= 0 else len(BIG_SEEDS)):
            for conn in (4, 8):
                for r, (min_area, largest) in enumerate(RULES):
                    out.append((f"{'big' if f < 0 else f}_{p}_{conn}_{r}", f, p, conn, min_area, largest))
    return out


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)
