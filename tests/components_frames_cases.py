"""Connected components on the bit planes of images of DIFFERENT sizes (include/la3d.h "connected components on bit planes",
la3d_components_bits_frames): the mixed-size case list the host and the GPU tests share.  The rule itself and its NumPy restatement
live in tests/components_cases.py; the sizes are those of the opening's mixed list (tests/open_bits_frames_cases.py)."""
import numpy as np

from . import components_cases as CC
from . import open_bits_frames_cases as FC

# one image each: (1, 1) to (140, 96), widths around a word, rows whose W is no multiple of 32 (the pitch is): the smallest shapes at
# which the per-row geometry, the word seams and the refusals can go wrong
SIZES = FC.SIZES
PER_IMAGE = 2
IMAGE_INDEX = np.repeat(np.arange(len(SIZES)), PER_IMAGE).astype(np.int32)
KINDS = tuple(CC.PATTERNS) + (("blob", None),)         # the patterns sized to each image, plus blob_plane
CONNECTIVITIES = (4, 8)
RULES4 = ((0, False), (CC.MIN_AREA, False), (0, True), (CC.MIN_AREA, True))   # (min_area, largest)
TABLE_ROWS = 8
SEED = 31
REFUSED = [-2, 0, 0, 0, 0, 0, 0, 0]

_CASES = []
_MEMO = {}


def cases():
    """-> the 24 (name, (H, W) bool plane) of the call, two per image in image order; plane n has kind n % 11, so every kind is seen
    on two or three sizes.  A pattern too dense for its frame fills only the frame's lower right 60 x 100 corner (the rule of
    components_cases.pattern_cases).  Made once, shared, never changed."""
    if not _CASES:
        rs = np.random.RandomState(SEED)
        for n, p in enumerate(IMAGE_INDEX):
            H, W = SIZES[p]
            name, fn = KINDS[n % len(KINDS)]
            m = CC.blob_plane(rs, H, W) if fn is None else fn(H, W)
            if CC.count_runs(m) > CC.MAX_CASE_RUNS:
                h, w = min(H, 60), min(W, 100)
                m = np.zeros((H, W), bool)
                m[H - h:, W - w:] = fn(h, w)
            assert CC.count_runs(m) <= CC.MAX_CASE_RUNS, (name, H, W)
            m.setflags(write=False)
            _CASES.append((f"{name}_{H}x{W}", m))
    return list(_CASES)


def planes():
    return [m for _, m in cases()]


def labelled(key, mask, conn):
    """the restatement's labelling of a plane, made once per (key, connectivity)"""
    if (key, conn) not in _MEMO:
        labels, n = CC.label(mask, conn)
        _MEMO[key, conn] = labels, n, CC.table_of(labels, n)
    return _MEMO[key, conn]


def expected(conn, min_area, largest, rows=TABLE_ROWS, named=None, max_runs=None):
    """what one call gives for the planes ``named`` (default: the case list) -> (outs: list of bool planes, stats int32 (B, 8), tables
    int32 (B, rows, 5)); a plane with more than ``max_runs`` runs: -1, runs, 0, ..., an all-zero plane, zero table rows"""
    named = cases() if named is None else named
    outs, stats, tabs = [], [], []
    for key, m in named:
        runs = CC.count_runs(m)
        tab = np.zeros((rows, 5), np.int32)
        if max_runs is not None and runs > max_runs:
            outs.append(np.zeros(m.shape, bool)); stats.append([-1, runs, 0, 0, 0, 0, 0, 0]); tabs.append(tab)
            continue
        labels, n, table = labelled(key, m, conn)
        out, st = CC.choose(labels, n, table, min_area, largest)
        tab[:min(n, rows)] = table[:rows]
        outs.append(out); stats.append(st); tabs.append(tab)
    return outs, np.asarray(stats, np.int32).reshape(len(named), 8), np.stack(tabs) if tabs else np.zeros((0, rows, 5), np.int32)


stacks = FC.stacks
frame_words = FC.frame_words
plane_words = FC.plane_words
