"""The NumPy restatement of mask overlap on bit planes (include/la3d.h "mask overlap on bit planes") and the cases its CPU and GPU
tests share.  Everything here is exact: counts are integers, the ratios one float64 division, the NMS rule one float64 multiply."""
import numpy as np

TILE, STEP = 8, 1024          # planes per side of a tile; the words a chunk is a whole multiple of
MIRROR, AREA_A, AREA_B = 1, 2, 4


def padded(w: int) -> int:
    return (w + 31) // 32 * 32


def plane_words(H: int, W_stored: int) -> int:
    return (H * W_stored + 31) // 32


def blobs(seed: int, n: int, H: int, W: int) -> np.ndarray:
    """n boolean masks (n, H, W): random rectangles and elliptic blobs, some of them unions of two"""
    rs = np.random.RandomState(seed)
    vv, uu = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), bool)
    for i in range(n):
        for _ in range(1 + rs.randint(2)):
            if rs.rand() < 0.5:
                h, w = rs.randint(1, H + 1), rs.randint(1, W + 1)
                r0, c0 = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
                out[i, r0:r0 + h, c0:c0 + w] = True
            else:
                cy, cx = rs.uniform(0, H), rs.uniform(0, W)
                ry, rx = rs.uniform(1, H / 2 + 1), rs.uniform(1, W / 2 + 1)
                out[i] |= ((vv - cy) / ry) ** 2 + ((uu - cx) / rx) ** 2 <= 1.0
    return out


def with_specials(masks: np.ndarray, seed: int = 0) -> np.ndarray:
    """the same stack with, where it has the rows for them: an all-ones plane (0), an empty plane (1), an identical pair (2, 3) and a
    nested pair (5 inside 4)"""
    m = masks.copy()
    n, H, W = m.shape
    if n >= 1:
        m[0] = True
    if n >= 2:
        m[1] = False
    if n >= 4:
        m[3] = m[2]
    if n >= 6:
        m[4] = False
        m[4, H // 8:H - H // 8, W // 8:W - W // 8] = True
        m[5] = False
        m[5, H // 4:H - H // 4, W // 4:W - W // 4] = True
    return m


def overlap_ref(A: np.ndarray, B: np.ndarray):
    """boolean (na, H, W), (nb, H, W) -> inter int64 (na, nb), area_a (na,), area_b (nb,)"""
    inter = (A[:, None] & B[None]).sum((-2, -1), dtype=np.int64) if len(A) and len(B) else np.zeros((len(A), len(B)), np.int64)
    return inter, A.sum((-2, -1), dtype=np.int64), B.sum((-2, -1), dtype=np.int64)


def ratio_ref(inter, area_a, area_b, kind: str) -> np.ndarray:
    """float64: inter / den with den by kind, 0.0 where den == 0"""
    aa, ab = np.broadcast_arrays(np.asarray(area_a, np.int64)[:, None], np.asarray(area_b, np.int64)[None, :])
    den = {"iou": aa + ab - inter, "iom": np.minimum(aa, ab), "ioa": aa + 0 * ab}[kind]
    out = np.zeros(inter.shape, np.float64)
    nz = den != 0
    out[nz] = inter[nz].astype(np.float64) / den[nz].astype(np.float64)
    return out


def nms_ref(inter, area, scores, thr: float, labels=None, kind: str = "iou") -> np.ndarray:
    """greedy NMS of ONE group, a plain loop: rows by descending score, ties to the lower row, NaN scores never visited; a kept row t
    suppresses a later row u iff the labels agree (or there are none), den > 0 and float64(inter) > thr * float64(den)"""
    n = len(area)
    scores = np.asarray(scores, np.float64)
    order = sorted((i for i in range(n) if not np.isnan(scores[i])), key=lambda i: (-scores[i], i))
    keep, gone = np.zeros(n, bool), np.zeros(n, bool)
    for k, t in enumerate(order):
        if gone[t] or area[t] < 0:
            continue
        keep[t] = True
        for u in order[k + 1:]:
            if gone[u] or area[u] < 0 or (labels is not None and labels[t] != labels[u]):
                continue
            den = min(int(area[t]), int(area[u])) if kind == "iom" else int(area[t]) + int(area[u]) - int(inter[t, u])
            if den > 0 and np.float64(inter[t, u]) > np.float64(thr) * np.float64(den):
                gone[u] = True
    return keep


def covered(tiles, counts_a, counts_b, group_words):
    """brute force over a tile table: how often each (group, i, j, word) of the call is covered -> one int array (na, nb, nw) per
    group; the self form (counts_b None) counts a mirror tile for both (i, j) and (j, i)"""
    self_form = counts_b is None
    cb = counts_a if self_form else counts_b
    cover = [np.zeros((int(a), int(b), int(w)), np.int32) for a, b, w in zip(counts_a, cb, group_words)]
    for t in tiles:
        c = cover[int(t["g"])]
        i0, j0, ni, nj, w0, w1 = (int(t[k]) for k in ("i0", "j0", "ni", "nj", "w0", "w1"))
        c[i0:i0 + ni, j0:j0 + nj, w0:w1] += 1
        if int(t["flags"]) & MIRROR:
            assert self_form
            c[j0:j0 + nj, i0:i0 + ni, w0:w1] += 1
    return cover


def rle_counts(mask) -> list:
    """uncompressed COCO run lengths of one boolean mask (column-major, zeros first)"""
    flat = np.asarray(mask, bool).ravel(order="F")
    edges = np.concatenate([[0], np.flatnonzero(flat[1:] != flat[:-1]) + 1, [flat.size]])
    return ([0] if flat[0] else []) + np.diff(edges).tolist()


def groups_ref(A, B, counts_a, counts_b, kind=None):
    """the flat outputs of a grouped call from boolean stacks whose groups are contiguous: inter (int64, ragged row-major), area_a,
    area_b, offsets - and the flat float64 ratio with ``kind``"""
    ra, rb = np.concatenate([[0], np.cumsum(counts_a)]), np.concatenate([[0], np.cumsum(counts_b)])
    inter, ratio, offsets = [], [], [0]
    area_a, area_b = A.sum((-2, -1), dtype=np.int64), B.sum((-2, -1), dtype=np.int64)
    for g in range(len(counts_a)):
        i, aa, ab = overlap_ref(A[ra[g]:ra[g + 1]], B[rb[g]:rb[g + 1]])
        inter.append(i.reshape(-1))
        if kind:
            ratio.append(ratio_ref(i, aa, ab, kind).reshape(-1))
        offsets.append(offsets[-1] + i.size)
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)   # noqa: E731
    return cat(inter, np.int64), area_a, area_b, np.asarray(offsets, np.int64), (cat(ratio, np.float64) if kind else None)
