"""Inputs and the NumPy restatement shared by tests/test_instance_points_contract.py (CPU) and tests/test_gpu_instance_points.py:
the masks every frame is tested with, depth planes with the special values, and the count / offset / sample rule of
``instance_points`` (include/la3d.h "instance point clouds") written with NumPy on top of the oracle's ``depth_to_points``."""
import numpy as np

from oracle import la3d_oracle as O

NSAMPLE = 500
FRAMES = ((5, 13), (33, 47), (96, 224), (100, 214), (480, 640))
MASK_NAMES = ("empty", "first pixel", "last pixel", "full", "row", "column", "checkerboard", "random 2 %", "runs over 31|32 and 63|64",
              "blob > 64")


def standard_masks(H, W, seed=0):
    """The ten masks of a frame, in the order of MASK_NAMES."""
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
    m[7, rs.randint(0, H), W - 1] = m[7, rs.randint(0, H), W - 2] = m[7, rs.randint(0, H), W - 3] = True   # the last three image columns
    flat = m[8].reshape(-1)
    flat[28:36] = True; flat[60:68] = True                                  # word boundaries of the flat (unpadded) bit plane
    if W > 68:
        m[8, H // 2, 28:36] = True; m[8, H // 2, 60:68] = True              # and of a row (padded pitch)
        m[8, H - 1, 30:34] = True
    flat = m[9].reshape(-1)
    start = max(0, min(W + 3, H * W - 100))
    flat[start:min(H * W, start + 100)] = True
    return m


def special_depth(P, H, W, seed=1):
    """P float32 planes of 0.5 .. 10 m with a NaN, an inf, a -inf, a zero and a negative depth in each (where the frame has room)."""
    rs = np.random.RandomState(seed)
    d = rs.uniform(0.5, 10.0, (P, H, W)).astype(np.float32)
    for p in range(P):
        f = d[p].reshape(-1)
        for k, val in enumerate((np.nan, np.inf, 0.0, -1.25, -np.inf)):
            f[(7 + 11 * k + 3 * p) % f.size] = val
    return d


def cameras(P, H, W):
    return np.stack([np.array([[0.8 * W + 3.5 * p, 0.0, W / 2.0 + 0.25 * p], [0.0, 0.9 * W - 2.0 * p, H / 2.0 - 0.5 * p], [0.0, 0.0, 1.0]])
                     for p in range(P)])


def cloud_rule(depth, masks, K, image_index=None, sample_idx=None, frame_width=None):
    """-> (points (T,3) f64, pixels (T,) i32, offsets (B+1,) i64, counts (B,) i32): per instance ``depth_to_points(depth[img][None],
    K[img])[mask]`` - NumPy's row-major order -, with sample_idx the rows ``cloud[sample_idx[n]]`` for a cloud of more than 500 points
    (a rank outside the cloud: a NaN row, pixel -1), packed by the exclusive prefix of the row counts."""
    depth = np.asarray(depth)
    depth = depth[None] if depth.ndim == 2 else depth
    K = np.asarray(K, np.float64)
    K = K[None] if K.ndim == 2 else K
    masks = np.asarray(masks).astype(bool)
    B, H, W = masks.shape
    fw = W if frame_width is None else frame_width
    pts, pix, counts = [], [], np.zeros(B, np.int32)
    for n in range(B):
        img = int(image_index[n]) if image_index is not None else (n if depth.shape[0] > 1 else 0)
        m = masks[n].copy()
        m[:, fw:] = False
        cloud = O.depth_to_points(depth[img][None], K[img if K.shape[0] > 1 else 0])[m]
        v, u = np.nonzero(m)
        px = (v * fw + u).astype(np.int32)
        counts[n] = len(cloud)
        if sample_idx is not None and len(cloud) > NSAMPLE:
            r = np.asarray(sample_idx[n]).astype(np.int64)
            ok = (r >= 0) & (r < len(cloud))
            sel, spx = np.full((NSAMPLE, 3), np.nan), np.full(NSAMPLE, -1, np.int32)
            sel[ok], spx[ok] = cloud[r[ok]], px[r[ok]]
            cloud, px = sel, spx
        pts.append(cloud.reshape(-1, 3)); pix.append(px)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64)
    return np.concatenate(pts) if B else np.zeros((0, 3)), np.concatenate(pix) if B else np.zeros(0, np.int32), offsets, counts
