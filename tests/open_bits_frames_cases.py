"""Morphology on the bit planes of images of DIFFERENT sizes (include/la3d.h "morphology on bit planes", la3d_open_bits_frames): the
mixed-size case list the host and the GPU tests share.  The rule itself and its NumPy restatement live in tests/open_bits_cases.py."""
import numpy as np

from . import open_bits_cases as OC

# one image each: widths around a word and around the 128-column vector store; heights that, once upscaled, land on and around band
# edges of 32 and 64; (140, 96) has more rows than any band; (1, 1), (3, 100), (7, 31), (8, 33) have far fewer bands than the bound's
SIZES = ((1, 1), (7, 31), (33, 47), (40, 32), (8, 33), (65, 64), (96, 224), (140, 96), (16, 65), (3, 100), (64, 128), (32, 160))
PER_IMAGE = 2
KS = (3, 7, 15)
SCALES = (1, 2, 4)
IMAGE_INDEX = np.repeat(np.arange(len(SIZES)), PER_IMAGE).astype(np.int32)


def planes(k, s):
    """-> the 24 (H, W) bool planes of the call (k, s), two per image in image order"""
    rs = np.random.RandomState(23 + 100 * k + s)
    return [OC.blob_plane(rs, *SIZES[p]) for p in IMAGE_INDEX]


def stacks(masks, sizes=SIZES, per_image=PER_IMAGE):
    """planes in image order -> one (n, H, W) uint8 stack per image, what pack_mask_frames takes"""
    return [np.stack(masks[p * per_image:(p + 1) * per_image]).astype(np.uint8) for p in range(len(sizes))]


def frame_words(mask):
    """(H, W) bool -> the uint32 words of its plane in the frame table's layout: pitch padded(W)"""
    return OC.words(mask, OC.padded(mask.shape[1]))


def plane_words(H, W):
    return H * OC.padded(W) // 32
