"""The inputs of tests/test_frames_masks_contract.py (which checks them on the oracle alone, on the CPU) and of
tests/test_gpu_frames_masks.py: per image a stack of instance masks, as an instance-segmentation network hands them over, for the
seven frame sizes of tests/frames_bits_cases.py - the smallest at which the ragged mask packer can go wrong: widths 224 / 96 / 32 are
multiples of 16 and 32 (u8 planes in 16-byte groups), 75 / 45 / 333 make dense rows start on odd bytes, a (50, 75) u8 plane has 3750
bytes so the plane behind it starts off a 16-byte boundary, planes of 150 and 14 words end inside a 16-byte group of the output, and
(7, 45) / (8, 32) have fewer than 64 tiles.  The rows come in the shape tests/test_gpu_frames.py's helpers (``oracle_mix``) take."""
import numpy as np

from oracle import la3d_oracle as O

from . import frames_bits_cases as FC
from .frames_bits_cases import CELLS, SIZES
from .test_gpu_labels import blocky

SEEDS = (0, 1, 2)
NO_MASKS = 3        # the image without an instance: a (0, H, W) stack
EMPTY_IMAGE = 0     # gets one all-zero plane more: status 1
PIXEL_IMAGE = 2     # gets one single-pixel plane more: status 3
CANVAS_IMAGE = 1    # its stack is the top-left crop of a larger canvas: (50, 75) in rows 96 elements apart
CANVAS_EXTRA = (3, 21)


def make_case(seed):
    """-> dict: sizes, stacks (per image a bool (N_p, H_p, W_p) array, N_p = 0 for one image), depth, K, and - the rows in image order,
    the order ``pack_mask_frames`` gives them - masks, rles, img, expect (the status each row is there for); order: a permutation of
    the rows (the packer and the fit take rows whose image_index is not sorted); segs: None (no polygons)"""
    rs = np.random.RandomState(100 + seed)
    depth = [rs.uniform(0.5, 10, s).astype(np.float32) for s in SIZES]
    K = np.stack([np.array([[rs.uniform(0.7, 1.3) * w, 0, w / 2 + rs.uniform(-9, 9)], [0, rs.uniform(0.7, 1.3) * w, h / 2 + rs.uniform(-9, 9)], [0, 0, 1]])
                  for h, w in SIZES])
    stacks, masks, img, expect = [], [], [], []
    for p, (h, w) in enumerate(SIZES):
        cells = blocky(rs, h, w, CELLS, max(2, h // 6), max(4, w // 7))
        n = 0 if p == NO_MASKS else rs.randint(2, 6)
        planes = [cells == c for c in rs.permutation(CELLS)[:n]]
        status = [0] * n
        if p == EMPTY_IMAGE:
            planes.insert(1, np.zeros((h, w), bool))
            status.insert(1, 1)
        if p == PIXEL_IMAGE:
            one = np.zeros((h, w), bool)
            one[3, 4] = True
            planes.append(one)
            status.append(3)
        stacks.append(np.stack(planes) if planes else np.zeros((0, h, w), bool))
        masks += planes
        img += [p] * len(planes)
        expect += status
    return dict(sizes=list(SIZES), stacks=stacks, depth=depth, K=K, masks=masks, rles=[O.rle_encode(m) for m in masks], segs=None,
                img=np.asarray(img, np.int32), expect=np.asarray(expect, np.int32), order=rs.permutation(len(masks)))


def as_u8(stack, rs):
    """non-zero bytes of every kind where the mask is set"""
    return np.where(stack, rs.randint(1, 256, stack.shape), 0).astype(np.uint8)


def as_logits(stack, threshold, rs):
    """-> (float32 logits, the masks they mean): threshold +- 1 around the masks (exact in float16 and bfloat16 for thresholds 0 and
    0.5), and - whatever the mask said there - pixels that are NaN (bit 0), +inf (1), -inf (0) and EXACTLY the threshold (0: the rule
    is x > threshold)"""
    x = np.where(stack, np.float32(threshold + 1), np.float32(threshold - 1)).astype(np.float32)
    mean = stack.copy()
    flat, mflat = x.reshape(-1), mean.reshape(-1)
    if flat.size:
        pick = rs.permutation(flat.size)[:4 * max(1, flat.size // 16)].reshape(4, -1)
        for idx, (value, bit) in zip(pick, ((np.nan, False), (np.inf, True), (-np.inf, False), (threshold, False))):
            flat[idx] = value
            mflat[idx] = bit
    return x, mean


def canvas_of(stack, fill):
    """the stack as the top-left crop of a canvas CANVAS_EXTRA larger, everything outside the crop ``fill``: -> (canvas, crop view)"""
    n, h, w = stack.shape
    canvas = np.full((n, h + CANVAS_EXTRA[0], w + CANVAS_EXTRA[1]), fill, stack.dtype)
    canvas[:, :h, :w] = stack
    return canvas, canvas[:, :h, :w]


def expected_words(masks):
    """per row the words its plane must hold: frames_bits_cases.expected_words (np.packbits, LSB first, on rows zero-padded to the
    pitch) with every mask as a label map of its own whose id is 1"""
    return FC.expected_words([np.asarray(m, np.int64) for m in masks], range(len(masks)), [1] * len(masks))
