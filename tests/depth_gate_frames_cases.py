"""The depth gate on the bit planes of images of DIFFERENT sizes (include/la3d.h "depth gate on bit planes",
la3d_depth_gate_bits_frames): the case lists tests/test_depth_gate_frames_contract.py and tests/test_gpu_depth_gate_frames.py share.
No new rule is stated here: the oracle is ``depth_gate_cases.gate`` applied per row on that row's own (H, frame_width) image - for
16-bit depth on ``depth16_cases.upconvert`` of the stored words.  Nothing here needs a GPU."""
import functools

import numpy as np

from . import depth16_cases as D16
from . import depth_gate_cases as DG
from . import open_bits_frames_cases as OF

# 12 images from (1, 1) to (140, 96), two rows each: the smallest shapes at which per-row geometry, word seams and a last word that is
# partly outside the image can go wrong
SIZES = OF.SIZES
IMAGE_INDEX = OF.IMAGE_INDEX
B = len(IMAGE_INDEX)
DEPTH_KINDS = ("smooth", "constant", "levels", "ulps", "negative", "mixed", "invalid")
MASK_KINDS = ("empty", "one", "two", "odd", "even", "full", "half")
REFUSED_COUNTS = [-2, 0, 0]


def depth_kind(p):
    return DEPTH_KINDS[p % len(DEPTH_KINDS)]


def mask_kind(b):
    return MASK_KINDS[(b + b // len(MASK_KINDS)) % len(MASK_KINDS)]


@functools.lru_cache(maxsize=None)
def depth_maps():
    """one float32 (H, W) map per image, the depth kinds of ``depth_gate_cases`` rotating over the images"""
    out = []
    for p, (h, w) in enumerate(SIZES):
        d = DG.depth_kinds(np.random.RandomState(500 + p), h, w)[depth_kind(p)].copy()
        d.setflags(write=False)
        out.append(d)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def masks():
    """one bool (H, W) mask per row, the mask kinds of ``depth_gate_cases`` rotating over the rows"""
    out = []
    for b, p in enumerate(IMAGE_INDEX):
        m = DG.mask_kinds(np.random.RandomState(900 + b), *SIZES[p])[mask_kind(b)].copy()
        m.setflags(write=False)
        out.append(m)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def stored(variant):
    """the 16-bit maps of ``depth_maps()`` for one of ``depth16_cases.VARIANTS``, quantised with NumPy (never with a packer under test)"""
    dtype, scale, _ = variant
    return tuple(D16.quantise(d, dtype, scale) for d in depth_maps())


@functools.lru_cache(maxsize=None)
def upconverted(variant):
    _, scale, hole = variant
    return tuple(D16.upconvert(x, scale, hole) for x in stored(variant))


def gate_rows(depths, row_masks, image_index, **kw):
    """the oracle, row by row: -> (keeps [bool (H, W)], counts int32 (B, 3), levels float32 (B, 3))"""
    res = [DG.gate(depths[p], m, **kw) for m, p in zip(row_masks, image_index)]
    if not res:
        return [], np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32)
    return [r[0] for r in res], np.stack([r[1] for r in res]), np.stack([r[2] for r in res])


@functools.lru_cache(maxsize=None)
def expected(params_index, variant=None):
    """the oracle on the mixed list under DG.PARAMS[params_index]; ``variant``: on the up-converted planes of that 16-bit variant"""
    return gate_rows(depth_maps() if variant is None else upconverted(variant), masks(), IMAGE_INDEX, **DG.PARAMS[params_index])


def frame_words(mask):
    return OF.frame_words(mask)


def plane_words(h, w):
    return OF.plane_words(h, w)


# ---- the second list: both selection paths ---------------------------------------------------------------------------------------
# every 96 x 96 row of DG.big_planes() is an image of its own (each has its own depth), mixed with three small images - DG.FRAMES, two
# rows each over their smooth depth - in ONE table.  The bounds of that table are the big rows' own frame (96 x 96); BIG_BOUNDS states
# larger ones, under which every row's frame is smaller than the bounds.
SMALL = tuple((h, w) for h, w, _ in DG.FRAMES)
SMALL_ROWS = (3, 6)                                  # of DG.planes(h, w): smooth / odd and smooth / half
BIG_BOUNDS = (128, 128)


@functools.lru_cache(maxsize=None)
def big_list():
    """-> (sizes, depth maps, masks, image_index): a small image in front, between and behind the big ones"""
    _, bd, bm = DG.big_planes()
    sizes, depths, row_masks, ii = [], [], [], []

    def small(j):
        h, w = SMALL[j]
        _, d, m = DG.planes(h, w)
        sizes.append((h, w)); depths.append(d[0])
        for r in SMALL_ROWS:
            row_masks.append(m[r]); ii.append(len(sizes) - 1)

    small(0)
    for n in range(len(bd)):
        if n == len(bd) // 2:
            small(1)
        sizes.append(DG.BIG); depths.append(bd[n]); row_masks.append(bm[n]); ii.append(len(sizes) - 1)
    small(2)
    return tuple(sizes), tuple(depths), tuple(row_masks), np.asarray(ii, np.int32)


@functools.lru_cache(maxsize=None)
def big_expected(params_index):
    _, depths, row_masks, ii = big_list()
    return gate_rows(depths, row_masks, ii, **DG.PARAMS[params_index])


def stacks(row_masks, image_index, P):
    """rows in image order -> one (n, H, W) uint8 stack per image, what pack_mask_frames takes"""
    ii = np.asarray(image_index)
    assert (np.diff(ii) >= 0).all()
    return [np.stack([m for m, q in zip(row_masks, ii) if q == p]).astype(np.uint8) for p in range(P)]
