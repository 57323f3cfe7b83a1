"""Morphology on bit planes (include/la3d.h "morphology on bit planes"): the NumPy restatement of the rule and the case lists the host
and the GPU tests share.  ``opening`` is written from the rule as the header states it - zero-filled shifts, AND over the window along
x then y, OR along x then y -, not from SciPy's text; tests/golden/g19_opening.npz (make_golden_opening.py) holds what
``scipy.ndimage.binary_opening`` itself gives on ``fixture_cases()``."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_opening.npz")
FRAMES = ((33, 47), (96, 224), (140, 96))      # (H, W): unaligned rows; whole words per row; more rows than any band
KS = (3, 7, 15)
SCALES = (1, 2, 4)
PLANES = 4                                     # planes per (frame, k, s)
SEED = 19
SENTINEL = 0x5A5A5A5A


def shifted(m, d, axis):
    """m moved by d along axis, zeros coming in: out[i] = m[i + d]"""
    out = np.zeros_like(m)
    n = m.shape[axis]
    if abs(d) >= n:
        return out
    src = [slice(None)] * m.ndim
    dst = [slice(None)] * m.ndim
    if d >= 0:
        src[axis], dst[axis] = slice(d, n), slice(0, n - d)
    else:
        src[axis], dst[axis] = slice(0, n + d), slice(-d, n)
    out[tuple(dst)] = m[tuple(src)]
    return out


def window(m, r, axis, op):
    out = m.copy()
    for d in range(-r, r + 1):
        out = op(out, shifted(m, d, axis))
    return out


def upscale(mask, s):
    """nearest neighbour by an integer factor: U[v, u] = M[v // s, u // s]"""
    m = np.asarray(mask, bool)
    v, u = np.arange(m.shape[0] * s) // s, np.arange(m.shape[1] * s) // s
    return m[np.ix_(v, u)]


def opening(mask, k, s=1):
    """(H, W) bool -> (s*H, s*W) bool: the opening by ones((k, k)) of the x s upscale; pixels outside the image count as unset"""
    m = upscale(mask, s)
    r = k // 2
    e = window(window(m, r, 1, np.logical_and), r, 0, np.logical_and)
    return window(window(e, r, 1, np.logical_or), r, 0, np.logical_or)


def rect_stats(mask):
    """area, x, y, w, h: the tight box of the set pixels (cv2.boundingRect of a binary image), zeros for an empty mask"""
    m = np.asarray(mask, bool)
    if not m.any():
        return [0, 0, 0, 0, 0]
    rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    return [int(m.sum()), int(cols[0]), int(rows[0]), int(cols[-1] - cols[0] + 1), int(rows[-1] - rows[0] + 1)]


def crop_rule(x, y, w, h, crop_size=512, upscale=4, ratio=0.7):
    """the crop parameters from a rectangle, on Python numbers: int() truncates, / is float division"""
    if w <= 0:
        return [float("nan")] * 3
    side = int(max(w, h) / ratio)
    return [(x + (w - side) / 2) / upscale, (y + (h - side) / 2) / upscale, crop_size / side * upscale]


def blob_plane(rs, H, W, noise=0.02):
    """the union of three random rectangles or ellipses, XORed with salt noise"""
    m = np.zeros((H, W), bool)
    vv, uu = np.mgrid[0:H, 0:W]
    for _ in range(3):
        cy, cx = rs.randint(0, H), rs.randint(0, W)
        hy, hx = rs.randint(1, max(2, H // 2)), rs.randint(1, max(2, W // 2))
        if rs.rand() < 0.5:
            m |= (np.abs(vv - cy) <= hy) & (np.abs(uu - cx) <= hx)
        else:
            m |= ((vv - cy) / float(hy)) ** 2 + ((uu - cx) / float(hx)) ** 2 <= 1.0
    return m ^ (rs.rand(H, W) < noise)


def fixture_cases():
    """-> list of (frame index, k, s); each has PLANES planes, in the order of fixture_planes()"""
    return [(f, k, s) for f in range(len(FRAMES)) for k in KS for s in SCALES]


def fixture_planes():
    """-> list, per case, of the (PLANES, H, W) bool inputs"""
    rs = np.random.RandomState(SEED)
    return [np.stack([blob_plane(rs, *FRAMES[f]) for _ in range(PLANES)]) for f, _, _ in fixture_cases()]


def random_cases(seed, n):
    """n cases (mask, k, s) over H in 1..70, W in 1..100, every k of the list, every factor and four densities"""
    rs = np.random.RandomState(seed)
    ks, dens = (1, 3, 5, 7, 9, 15, 31), (0.5, 0.9, 0.97, 0.995)
    out = []
    for i in range(n):
        H, W = rs.randint(1, 71), rs.randint(1, 101)
        out.append((rs.rand(H, W) < dens[i % 4], ks[i % 7], SCALES[(i // 7) % 3]))
    return out


def words(mask, W_out):
    """(H, W) bool -> the uint32 words of its plane stored W_out wide"""
    H, W = mask.shape
    m = np.zeros((H, W_out), bool)
    m[:, :W] = mask
    flat = m.reshape(-1)
    pad = (-len(flat)) % 32
    return np.packbits(np.concatenate([flat, np.zeros(pad, bool)]), bitorder="little").view(np.uint32)


def padded(W):
    return (W + 31) // 32 * 32


def pack(masks):
    """(N, H, W) bool -> (N, ceil(H*W/8)) uint8, little bit order (what the fixture stores)"""
    m = np.asarray(masks, bool)
    return np.packbits(m.reshape(len(m), -1), axis=1, bitorder="little")


def unpack(packed, H, W):
    return np.unpackbits(packed, axis=1, bitorder="little")[:, :H * W].reshape(len(packed), H, W).astype(bool)


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_case(g, i):
    """-> (inputs (PLANES, H, W), SciPy's outputs (PLANES, s*H, s*W)) of fixture case i"""
    f, k, s = fixture_cases()[i]
    H, W = FRAMES[f]
    return unpack(g[f"in_{i}"], H, W), unpack(g[f"out_{i}"], s * H, s * W)
