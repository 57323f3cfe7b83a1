"""Crop-space masks as bit planes (include/la3d.h "crop-space masks as bit planes"): the NumPy restatement of the rule and the case
lists the host and the GPU tests share.  ``restore`` is written from the rule as the header states it, not from the reference's
text: per pixel of the frame, in float64, one multiply and a floor.  tests/golden/g18_crops.npz (make_golden_crops.py) holds what
the reference's own ``restore_mask_from_crop`` gives on ``fixture_cases()``."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_crops.npz")
S_FIX = 16
FRAMES = ((33, 47), (96, 224))           # (H, W): an odd width that is no multiple of 32, and whole words per row
SENTINEL = 0x5A5A5A5A
SIDE_MAX = 1 << 20                       # the bound la3d.h states for `side`


def placement(ox, oy, s, S):
    """x1, y1, side on Python floats: round half to even, int() truncates"""
    return int(round(float(ox))), int(round(float(oy))), int(int(S) / float(s))


def restore(resized_mask, ox, oy, s, shape):
    """the rule: bit (v, u) = crop[sy][sx] != 0 where x1 <= u < x1 + side, y1 <= v < y1 + side inside the frame; an empty mask for
    side <= 0 (and > SIDE_MAX) and for a placement wholly outside the frame"""
    m = np.asarray(resized_mask)
    S = m.shape[0]
    H, W = int(shape[0]), int(shape[1])
    x1, y1, side = placement(ox, oy, s, S)
    return restore_placed(m != 0, x1, y1, side, H, W)


def restore_placed(m, x1, y1, side, H, W):
    out = np.zeros((H, W), bool)
    S = m.shape[0]
    if side <= 0 or side > SIDE_MAX:
        return out
    ifx = 1.0 / (float(side) / float(S))
    u, v = np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64)
    inu, inv = (u >= x1) & (u < x1 + side), (v >= y1) & (v < y1 + side)
    if not inu.any() or not inv.any():
        return out
    sx = np.minimum(np.floor((u[inu] - x1).astype(np.float64) * ifx).astype(np.int64), S - 1)
    sy = np.minimum(np.floor((v[inv] - y1).astype(np.float64) * ifx).astype(np.int64), S - 1)
    out[np.ix_(inv, inu)] = m[np.ix_(sy, sx)]
    return out


def fixture_cases():
    """-> list of (name, frame index, offset_x, offset_y, scale_factor); S = S_FIX.  side = int(16 / scale)."""
    cases = []
    for f, (H, W) in enumerate(FRAMES):
        up = 16 / 37.0                                  # side 37 (or 36: int() decides)
        sd_up = int(16 / up)
        cases += [
            (f"up_{f}", f, 3.0, 2.0, 16 / 21.0), (f"down_{f}", f, 11.0, 7.0, 2.3), (f"same_{f}", f, 5.0, 9.0, 1.0),
            (f"half_even_{f}", f, 2.5, 4.5, 0.8), (f"half_odd_{f}", f, 3.5, 5.5, 0.8), (f"half_neg_{f}", f, -2.5, -3.5, 0.8),
            (f"half_neg_odd_{f}", f, -3.5, -2.5, 1.25),
            (f"over_left_{f}", f, -9.0, 4.0, 0.8), (f"over_top_{f}", f, 6.0, -11.0, 0.8),
            (f"over_right_{f}", f, W - 8.5, 3.0, 0.8), (f"over_bottom_{f}", f, 4.0, H - 7.5, 0.8),
            (f"corner_tl_{f}", f, -7.5, -6.5, 0.8), (f"corner_br_{f}", f, W - 9.0, H - 5.0, 0.8),
            (f"over_all_{f}", f, -20.0, -30.0, 16.0 / (2 * W + 61)),
            (f"out_left_{f}", f, -23.0, 4.0, 0.8), (f"out_left_touch_{f}", f, -20.0, 4.0, 0.8),
            (f"out_right_{f}", f, W + 2.0, 4.0, 0.8), (f"out_right_touch_{f}", f, float(W), 4.0, 0.8),
            (f"out_top_{f}", f, 4.0, -21.0, 0.8), (f"out_bottom_{f}", f, 4.0, H + 5.0, 0.8),
            (f"out_corner_{f}", f, W + 1.0, H + 1.0, 0.8),
            (f"side1_{f}", f, 7.0, 8.0, 16.0), (f"side1_frac_{f}", f, W - 1.0, H - 1.0, 10.0), (f"side0_{f}", f, 7.0, 8.0, 17.0),
            (f"up_overhang_{f}", f, -sd_up + 4.5, H - 6.5, up),
        ]
    return cases


def fixture_crops():
    """the (N, S, S) u8 crops of fixture_cases(): seeded, about half set, values 0 / 1; pixel (0, 0) - all a side of 1 shows - is set"""
    rs = np.random.RandomState(18)
    crops = (rs.rand(len(fixture_cases()), S_FIX, S_FIX) < 0.5).astype(np.uint8)
    crops[:, 0, 0] = 1
    return crops


def random_batch(seed, B, S, H, W):
    """-> (crops (B, S, S) u8 0 / 1, params (B, 3) float64): sides from 1 to twice the frame, offsets that overhang every border,
    half of them ending in .5; the last two rows lie outside the frame / have side 0"""
    rs = np.random.RandomState(seed)
    crops = (rs.rand(B, S, S) < 0.5).astype(np.uint8)
    side = rs.randint(1, 2 * max(H, W), B)
    side[0], side[1] = S, 1
    scale = S / side.astype(np.float64)
    ox = rs.randint(-side, W + 1).astype(np.float64) * 0.6 + (rs.rand(B) < 0.5) * 0.5
    oy = rs.randint(-side, H + 1).astype(np.float64) * 0.6 + (rs.rand(B) < 0.5) * 0.5
    ox, oy = np.round(ox * 2) / 2, np.round(oy * 2) / 2
    ox[B - 2], scale[B - 1] = W + 3.0, S + 1.0
    return crops, np.stack([ox, oy, scale], 1)


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


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_masks(g):
    """-> the list of expected (H, W) bool masks of the fixture cases, in case order"""
    out, at = [], [0] * len(FRAMES)
    for f in g["frame"]:
        out.append(g[f"out_{f}"][at[f]].astype(bool))
        at[f] += 1
    return out
