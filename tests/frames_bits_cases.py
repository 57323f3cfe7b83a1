"""The inputs of tests/test_frames_bits_contract.py (which checks them on the oracle alone, on the CPU) and of
tests/test_gpu_frames_bits.py: label maps of seven sizes, the (image, id) rows asked of them and the masks those rows mean - in the
shape tests/test_gpu_frames.py's helpers (``oracle_mix``) take."""
import numpy as np

from .test_gpu_labels import blocky, encode

# (H, W): pitches 224 / 96 / 64 / 96 / 352 / 32 / 512; planes of 150 (50 x 96 / 32) and 14 (7 x 64 / 32) words end in the middle of a
# 16-byte group; (7, 45) and (8, 32) have fewer than 64 tiles of 32 x 8 pixels (2 and 1)
SIZES = [(96, 224), (50, 75), (7, 45), (64, 96), (120, 333), (8, 32), (37, 500)]
SEEDS = (0, 1, 2)
CELLS = 5
NO_IDS = 3          # the image nothing is asked of
ABSENT_ID = 200     # no map holds it: an empty plane, status 1
PIXEL_ID = 77       # one pixel of image 1 holds it: status 3


def pitch(w):
    return (w + 31) // 32 * 32


def make_case(seed, dtype="u8"):
    """-> dict: sizes, values (true ids, int64 (H, W) per image), maps (what a caller holds: ``dtype``), ids (per image), depth, K,
    and - the rows in ``ids`` order - masks, img, expect (the status each row is there for)"""
    rs = np.random.RandomState(seed)
    values = [blocky(rs, h, w, CELLS, max(2, h // 6), max(4, w // 7)) + 1 for h, w in SIZES]   # cell c has id c + 1
    depth = [rs.uniform(0.5, 10, s).astype(np.float32) for s in SIZES]
    K = np.stack([np.array([[rs.uniform(0.7, 1.3) * w, 0, w / 2 + rs.uniform(-9, 9)], [0, rs.uniform(0.7, 1.3) * w, h / 2 + rs.uniform(-9, 9)], [0, 0, 1]])
                  for h, w in SIZES])
    values[1][3, 4] = PIXEL_ID
    ids = [[] if p == NO_IDS else list(range(1, CELLS + 1)) for p in range(len(SIZES))]
    ids[0].append(ABSENT_ID)
    ids[1].append(PIXEL_ID)
    masks, img, expect = [], [], []
    for p, row in enumerate(ids):
        for i in row:
            masks.append(values[p] == i)
            img.append(p)
            expect.append(1 if i == ABSENT_ID else 3 if i == PIXEL_ID else 0)
    return dict(sizes=list(SIZES), values=values, maps=[encode(v, dtype) for v in values], ids=ids, depth=depth, K=K, masks=masks, segs=None,
                img=np.asarray(img, np.int32), expect=np.asarray(expect, np.int32))


def expected_words(values, img, flat_ids):
    """per row the words its plane must hold: np.packbits, LSB first, of ``values[image] == id`` on rows zero-padded to the pitch"""
    out = []
    for p, i in zip(img, flat_ids):
        h, w = values[p].shape
        m = np.zeros((h, pitch(w)), bool)
        m[:, :w] = values[p] == i
        out.append(np.packbits(m.reshape(-1), bitorder="little").view(np.uint32))
    return out
