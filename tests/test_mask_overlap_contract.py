"""CPU-only tests of mask overlap on bit planes (include/la3d.h "mask overlap on bit planes"): the names on every layer, the tile
table of la3d_mask_overlap_plan by brute force, the workspace size, the limits and the refusals of the C entries before any launch
(fake pointers: nothing here reaches a device), the Python argument errors, and the NumPy restatement on cases worked by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import mask_overlap_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2


def test_names_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _lib, overlap

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    assert "mask overlap on bit planes" in hdr
    for fn in ("la3d_mask_overlap_plan", "la3d_mask_overlap_workspace_bytes", "la3d_mask_overlap", "la3d_mask_nms"):
        assert re.search(r"\b%s\s*\(" % fn, hdr) and fn in _lib.EXPORTS and hasattr(_lib.lib, fn), fn
    for fn in ("mask_overlap", "mask_iou", "mask_nms", "mask_overlap_plan", "MaskOverlap", "OverlapPlan"):
        assert fn in la.__all__ and getattr(overlap, fn) is getattr(la, fn), fn
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2     # additive
    assert C.sizeof(_lib.OverlapTile) == 64 == overlap.TILE_DTYPE.itemsize
    assert C.sizeof(_lib.MaskOverlapArgs) == 208 and _lib.MaskOverlapArgs.tiles.offset == 136
    assert C.sizeof(_lib.MaskNmsArgs) == 96 and _lib.MaskNmsArgs.thr.offset == 72
    for name, _ in _lib.OverlapTile._fields_:
        assert overlap.TILE_DTYPE.fields[name][1] == getattr(_lib.OverlapTile, name).offset, name
    assert (_lib.OVERLAP_TILE, _lib.OVERLAP_STEP) == (MC.TILE, MC.STEP)
    assert (_lib.OVERLAP_MIRROR, _lib.OVERLAP_AREA_A, _lib.OVERLAP_AREA_B) == (MC.MIRROR, MC.AREA_A, MC.AREA_B)
    for name, v in (("NONE", 0), ("IOU", 1), ("IOM", 2), ("IOA", 3)):
        assert re.search(r"#define LA3D_OVERLAP_%s %d\b" % (name, v), hdr) and getattr(_lib, "OVERLAP_" + name) == v


COUNTS = [0, 1, 7, 8, 9, 17, 3, 0, 8, 1, 17, 0]
OTHER = [1, 0, 9, 8, 7, 3, 17, 0, 1, 17, 0, 8]
WORDS = [49, 1023, 1024, 1025, 2048, 2049, 0, 5, 3000, 1, 700, 4097]


def check_table(tiles, offsets, ca, cb, words):
    """every (group, i, j, word) in exactly one tile; the offsets; the fields the kernels rely on"""
    other = ca if cb is None else cb
    assert offsets.tolist() == np.concatenate([[0], np.cumsum(np.asarray(ca, np.int64) * np.asarray(other, np.int64))]).tolist()
    for c in MC.covered(tiles, ca, cb, words):
        assert (c == 1).all()
    ra, rb = np.concatenate([[0], np.cumsum(ca)]), np.concatenate([[0], np.cumsum(other)])
    area_a, area_b = np.zeros(ra[-1], int), np.zeros(rb[-1], int)
    for n, t in enumerate(tiles):
        g = int(t["g"])
        assert 0 <= t["ni"] <= MC.TILE and 0 <= t["nj"] <= MC.TILE and t["ni"] + t["nj"] > 0
        assert t["i0"] % MC.TILE == 0 and t["j0"] % MC.TILE == 0 and t["i0"] + t["ni"] <= ca[g] and t["j0"] + t["nj"] <= other[g]
        assert t["row_a"] == ra[g] + t["i0"] and t["row_b"] == rb[g] + t["j0"]
        assert t["nw"] == words[g] and t["nb"] == other[g] and t["out0"] == offsets[g]
        assert t["w0"] % MC.STEP == 0 and t["w0"] <= t["w1"] <= t["nw"] and (t["w1"] == t["nw"] or t["w1"] % MC.STEP == 0)
        assert 0 <= t["chunk"] < t["nchunks"]
        first = tiles[n - int(t["chunk"])]                                 # the chunks of a tile follow each other
        assert first["chunk"] == 0 and all(first[k] == t[k] for k in ("g", "i0", "j0", "ni", "nj", "nchunks", "flags"))
        if cb is None:
            assert t["j0"] >= t["i0"] and bool(t["flags"] & MC.MIRROR) == (t["j0"] > t["i0"])
        if t["chunk"] == 0:
            if t["flags"] & MC.AREA_A:
                area_a[t["row_a"]:t["row_a"] + t["ni"]] += 1
            if t["flags"] & MC.AREA_B:
                area_b[t["row_b"]:t["row_b"] + t["nj"]] += 1
    assert (area_a == 1).all() and (area_b == 1).all()                     # every area has exactly one writer


def test_plan_covers_every_pair_and_word_exactly_once():
    from labelany3d_amd.overlap import plan_tiles

    tiles, offsets = plan_tiles(COUNTS, OTHER, WORDS)
    check_table(tiles, offsets, COUNTS, OTHER, WORDS)
    assert len(tiles) < 1024 and tiles["nchunks"].max() > 1               # a small call: the words are split
    tiles, offsets = plan_tiles(COUNTS, None, WORDS)                      # the self form: on and above the diagonal
    check_table(tiles, offsets, COUNTS, None, WORDS)
    for nwords in (0, 1, 1023, 1024, 1025, 9600):
        for ca, cb in (([3], [3]), ([3], None), ([1, 7, 8, 9, 17], [17, 9, 8, 7, 1]), ([17, 9], None), ([0, 5], [4, 0])):
            tiles, offsets = plan_tiles(ca, cb, None, nwords)
            check_table(tiles, offsets, ca, cb, [nwords] * len(ca))
    tiles, offsets = plan_tiles([], None, None, 9600)
    assert len(tiles) == 0 and offsets.tolist() == [0]
    tiles, _ = plan_tiles([0, 0], [0, 0], None, 9600)
    assert len(tiles) == 0


def test_plan_splits_the_words_of_a_small_call_only():
    from labelany3d_amd.overlap import plan_tiles

    one, _ = plan_tiles([3], [3], None, 9600)                             # one 640 x 480 group, 3 x 3 rows: ten chunks of 1024 words
    assert len(one) == 10 and one["nchunks"].tolist() == [10] * 10 and one["w0"].tolist() == [1024 * c for c in range(10)]
    assert one["w1"].tolist() == [1024 * (c + 1) for c in range(9)] + [9600]
    hundred, _ = plan_tiles([100], None, None, 9600)                      # 91 tiles on and above the diagonal, split to fill the chip
    assert hundred["nchunks"].min() > 1 and len(hundred) == 91 * int(hundred["nchunks"][0])
    big, _ = plan_tiles([100] * 64, None, None, 9600)                     # 5824 tiles: nothing to split
    assert len(big) == 64 * 91 and (big["nchunks"] == 1).all() and (big["w1"] == 9600).all()


def test_plan_capacity_and_limits():
    from labelany3d_amd import _lib

    plan = _lib.lib.la3d_mask_overlap_plan
    ca, cb = np.array([9, 17], np.int32), np.array([8, 1], np.int32)
    offs = np.zeros(3, np.int64)
    p = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    n = plan(2, p(ca), p(cb), None, 49, None, 0, p(offs))
    assert n == 2 + 3 and offs.tolist() == [0, 72, 89]
    buf = np.zeros(n, np.dtype("V64"))
    assert plan(2, p(ca), p(cb), None, 49, p(buf), n, p(offs)) == n
    assert plan(2, p(ca), p(cb), None, 49, p(buf), n - 1, p(offs)) == -1 and b"smaller" in _lib.lib.la3d_last_error()
    assert plan(2, p(ca), p(cb), None, 49, p(buf), 0, p(offs)) == -1
    assert plan(-1, p(ca), p(cb), None, 49, None, 0, p(offs)) == ARG and plan(2, p(ca), p(cb), None, 49, None, 0, None) == ARG
    assert plan(2, p(ca), p(cb), None, -1, None, 0, p(offs)) == ARG
    assert plan(2, p(np.array([9, -1], np.int32)), p(cb), None, 49, None, 0, p(offs)) == ARG
    # H * W_stored <= 2^28 (2^23 words), at most 2^31 - 1 pairs: refused on the host, with a message
    assert plan(2, p(ca), p(cb), None, 1 << 23, None, 0, p(offs)) == 1025          # (5 tiles in 205 chunks each)
    assert plan(2, p(ca), p(cb), None, (1 << 23) + 1, None, 0, p(offs)) == UNSUPPORTED and b"2^23" in _lib.lib.la3d_last_error()
    gw = np.array([49, (1 << 23) + 1], np.int64)
    assert plan(2, p(ca), p(cb), p(gw), 0, None, 0, p(offs)) == UNSUPPORTED
    big = np.array([46340], np.int32)
    assert plan(1, p(big), None, None, 0, None, 0, p(offs)) > 0 and offs[1] == 46340 * 46340
    big[0] = 46341
    assert plan(1, p(big), None, None, 0, None, 0, p(offs)) == UNSUPPORTED and b"2^31 - 1" in _lib.lib.la3d_last_error()
    assert plan(2, p(np.array([40000, 40000], np.int32)), None, None, 0, None, 0, p(offs)) == UNSUPPORTED


def test_workspace_bytes():
    from labelany3d_amd import _lib

    ws = _lib.lib.la3d_mask_overlap_workspace_bytes
    assert ws(0) == 0 and ws(-3) == 0                                     # an empty call
    assert ws(1) == 320 and ws(10) == 3200 and ws(1 << 31) == 320 << 31   # 64 pair counts and 16 areas per tile; size_t
    from labelany3d_amd.overlap import plan_tiles

    assert ws(len(plan_tiles([], None, None, 9600)[0])) == 0


class Fake:
    """fake "device" memory, 64-byte aligned: every call below is refused, or has nothing to do, before any launch"""

    def __init__(self):
        self.buf = (C.c_char * 32768)()
        self.p = (C.addressof(self.buf) + 63) & ~63


def overlap_call(f, **kw):
    from labelany3d_amd import _lib

    a = dict(struct_size=C.sizeof(_lib.MaskOverlapArgs), G=1, kind=_lib.OVERLAP_IOU, rows_a=3, rows_b=3, a_bits=f.p, b_bits=f.p + 1024,
             a_stride=52, b_stride=52, nwords=49, tiles=f.p + 2048, ntiles=1, npairs=9, inter=f.p + 4096, area_a=f.p + 6144,
             area_b=f.p + 8192, iou=f.p + 10240, workspace=f.p + 12288)
    a.update(kw)
    rc = _lib.lib.la3d_mask_overlap(C.byref(_lib.MaskOverlapArgs(**a)))
    return rc, _lib.lib.la3d_last_error()


def test_overlap_entry_refuses_before_any_launch():
    from labelany3d_amd import _lib

    f = Fake()
    assert _lib.lib.la3d_mask_overlap(None) == ARG
    assert overlap_call(f, struct_size=200)[0] == ARG and overlap_call(f, struct_size=0)[0] == ARG
    for name in ("G", "rows_a", "rows_b", "ntiles", "npairs", "nwords"):
        assert overlap_call(f, **{name: -1})[0] == ARG, name
    assert overlap_call(f, kind=0)[0] == ARG and overlap_call(f, kind=4)[0] == ARG and overlap_call(f, kind=0, iou=None, ntiles=0)[0] == 0
    for name in ("a_bits", "tiles", "inter", "area_a", "area_b", "workspace"):
        assert overlap_call(f, **{name: None})[0] == ARG, name
    assert overlap_call(f, b_bits=None, area_b=None, rows_b=0, tiles=None)[0] == ARG   # (a side without rows needs no pointers: the next refusal)
    for name, at in (("a_bits", 0), ("b_bits", 1024), ("inter", 4096), ("area_a", 6144), ("area_b", 8192), ("workspace", 12288)):
        assert overlap_call(f, **{name: f.p + at + 2})[0] == ARG, name    # 4 bytes
    assert overlap_call(f, tiles=f.p + 2048 + 4)[0] == ARG and overlap_call(f, iou=f.p + 10240 + 4)[0] == ARG    # 8 bytes
    assert overlap_call(f, a_stride=48)[0] == ARG and overlap_call(f, b_stride=48)[0] == ARG
    # the limits need no device
    rc, msg = overlap_call(f, nwords=(1 << 23) + 1, a_stride=1 << 24, b_stride=1 << 24)
    assert rc == UNSUPPORTED and b"2^23" in msg
    rc, msg = overlap_call(f, npairs=1 << 31)
    assert rc == UNSUPPORTED and b"2^31 - 1" in msg
    # the frames form: group g is image g
    fr = dict(frames=f.p + 14336, P=1, H=8, W=32, a_offsets=f.p + 16384, b_offsets=f.p + 18432, a_image_index=f.p + 20480,
              b_image_index=f.p + 22528, a_words=64, b_words=64)
    assert overlap_call(f, **dict(fr, P=2))[0] == ARG and overlap_call(f, **dict(fr, H=0))[0] == ARG and overlap_call(f, **dict(fr, W=0))[0] == ARG
    assert overlap_call(f, **dict(fr, a_words=-1))[0] == ARG
    for name in ("a_offsets", "b_offsets", "a_image_index", "b_image_index"):
        assert overlap_call(f, **dict(fr, **{name: None}))[0] == ARG, name
    assert overlap_call(f, **dict(fr, a_bits=f.p + 4))[0] == ARG and overlap_call(f, **dict(fr, b_bits=f.p + 1024 + 8))[0] == ARG   # 16 bytes
    assert overlap_call(f, **dict(fr, a_offsets=f.p + 16384 + 4))[0] == ARG and overlap_call(f, **dict(fr, frames=f.p + 14336 + 4))[0] == ARG
    assert overlap_call(f, **dict(fr, a_image_index=f.p + 20480 + 2))[0] == ARG
    assert overlap_call(f, **dict(fr, H=1 << 14, W=(1 << 14) + 32))[0] == UNSUPPORTED
    # an empty call is success without a launch, whatever the pointers
    assert overlap_call(f, ntiles=0, npairs=0, a_bits=None, tiles=None, inter=None, area_a=None, area_b=None, workspace=None, b_bits=None)[0] == 0


def test_nms_entry_refuses_before_any_launch():
    from labelany3d_amd import _lib

    f = Fake()

    def call(**kw):
        a = dict(struct_size=C.sizeof(_lib.MaskNmsArgs), G=1, kind=_lib.OVERLAP_IOU, B=3, inter=f.p, area=f.p + 1024, offsets=f.p + 2048,
                 row_offsets=f.p + 4096, order=f.p + 6144, labels=None, thr=0.5, keep=f.p + 8192)
        a.update(kw)
        return _lib.lib.la3d_mask_nms(C.byref(_lib.MaskNmsArgs(**a)))

    assert _lib.lib.la3d_mask_nms(None) == ARG and call(struct_size=88) == ARG
    assert call(G=-1) == ARG and call(B=-1) == ARG
    assert call(kind=0) == ARG and call(kind=_lib.OVERLAP_IOA) == ARG
    assert call(thr=float("nan")) == ARG
    for name in ("inter", "area", "offsets", "row_offsets", "order", "keep"):
        assert call(**{name: None}) == ARG, name
    assert call(inter=f.p + 2) == ARG and call(order=f.p + 6144 + 2) == ARG and call(labels=f.p + 10240 + 2) == ARG and call(offsets=f.p + 2048 + 4) == ARG
    assert call(B=1 << 31) == UNSUPPORTED
    assert call(G=0) == 0 and call(B=0) == 0                              # nothing to do


def host_grid(sizes):
    import torch

    import labelany3d_amd as la
    from labelany3d_amd.frames import _bounds, frame_table, table_words

    t = frame_table(list(sizes))
    return la.FrameGrid(torch.as_tensor(table_words(t)), t, *_bounds(t), [tuple(s) for s in sizes])


def host_bits(grid, ii):
    import torch

    import labelany3d_amd as la

    offs, total = la.frame_bits_offsets(grid.table_host, ii)
    return la.FrameBits(torch.zeros(max(total, 4), dtype=torch.int32), torch.as_tensor(offs), torch.as_tensor(np.asarray(ii, np.int32)),
                        torch.zeros(len(ii), dtype=torch.int32), grid.table_host, grid.H, grid.W)


def test_python_argument_errors_come_before_any_device_work():
    import torch

    import labelany3d_amd as la

    def mb(n, H=33, W=47, Ws=64, fw=None):                                # on the host: never reaches a device
        return la.MaskBits(torch.zeros((n, MC.plane_words(H, Ws)), dtype=torch.int32), H, Ws, W if fw is None else fw)

    a, b = mb(5), mb(4)
    for fn in (la.mask_overlap, la.mask_overlap_plan):
        with pytest.raises(ValueError, match="MaskBits or a FrameBits"):
            fn((a.bits, 33, 64))
        with pytest.raises(ValueError, match="both be"):
            fn(a, host_bits(host_grid([(8, 32)]), [0]))
        with pytest.raises(ValueError, match="different frames"):
            fn(a, mb(4, H=34))
        with pytest.raises(ValueError, match="different frames"):
            fn(a, mb(4, Ws=47))
        with pytest.raises(ValueError, match="different frames"):
            fn(a, mb(4, fw=46))
        with pytest.raises(ValueError, match="sums to 4"):
            fn(a, b, counts_a=[2, 2], counts_b=[2, 2])
        with pytest.raises(ValueError, match="sums to 5"):
            fn(a, b, counts_a=[2, 3], counts_b=[2, 3])
        with pytest.raises(ValueError, match="2 groups and counts_b 3"):
            fn(a, b, counts_a=[2, 3], counts_b=[2, 1, 1])
        with pytest.raises(ValueError, match="1 groups and counts_b 2"):
            fn(a, b, counts_b=[2, 2])
        with pytest.raises(ValueError, match="negative"):
            fn(a, counts_a=[6, -1])
        with pytest.raises(ValueError, match="sequence of ints"):
            fn(a, counts_a=[2.5, 2.5])
        with pytest.raises(ValueError, match="sequence of ints"):
            fn(a, counts_a=torch.tensor([5]))
        with pytest.raises(ValueError, match="counts_b without b"):
            fn(a, counts_a=[5], counts_b=[5])
        with pytest.raises(ValueError, match="frames goes with FrameBits"):
            fn(a, frames=host_grid([(33, 47)]))
    for bad in ("IoU", "giou", 1, True):
        with pytest.raises(ValueError, match="iou must be"):
            la.mask_overlap(a, iou=bad)
    grid = host_grid([(33, 47), (96, 224), (140, 96)])
    fa, fb = host_bits(grid, [0, 0, 1, 2, 2, 2]), host_bits(grid, [0, 1, 1, 2])
    for fn in (la.mask_overlap, la.mask_overlap_plan):
        with pytest.raises(ValueError, match="need frames"):
            fn(fa, fb, counts_a=[2, 1, 3], counts_b=[1, 2, 1])
        with pytest.raises(ValueError, match="need frames"):
            fn(fa, fb, counts_a=[2, 1, 3], counts_b=[1, 2, 1], frames=grid.table_host)
        with pytest.raises(ValueError, match="another frame table"):
            fn(fa, fb, counts_a=[2, 1, 3], counts_b=[1, 2, 1], frames=host_grid([(33, 47), (96, 224), (140, 97)]))
        with pytest.raises(ValueError, match="need counts"):
            fn(fa, frames=grid)
        with pytest.raises(ValueError, match="need counts"):
            fn(fa, fb, counts_a=[2, 1, 3], frames=grid)
        with pytest.raises(ValueError, match="one entry per image"):
            fn(fa, counts_a=[3, 3], frames=grid)
        with pytest.raises(ValueError, match="sums to 5"):
            fn(fa, counts_a=[2, 1, 2], frames=grid)
    with pytest.raises(ValueError, match="on the GPU"):
        la.mask_overlap(a, b)                                             # the last check of all: where the planes live
    with pytest.raises(ValueError, match="on the GPU"):
        la.mask_overlap(fa, fb, counts_a=[2, 1, 3], counts_b=[1, 2, 1], frames=grid)
    plan = la.mask_overlap_plan(a, b, device="cpu")                       # the host tables of a plan need no device
    assert plan.tiles is None and len(plan.tiles_host) == 1 and plan.offsets.tolist() == [0, 20]
    with pytest.raises(ValueError, match="plan must be"):
        la.mask_overlap(a, b, plan=plan)
    # mask_nms
    s = np.zeros(5)
    for bad in ("ioa", None, "IoU"):
        with pytest.raises(ValueError, match="kind must be"):
            la.mask_nms(a, s, kind=bad)
    for bad in (float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="iou_threshold"):
            la.mask_nms(a, s, iou_threshold=bad)
    with pytest.raises(ValueError, match="scores must hold one value per row"):
        la.mask_nms(a, np.zeros(4))
    with pytest.raises(ValueError, match="labels must hold one value per row"):
        la.mask_nms(a, s, labels=np.zeros(6, np.int32))
    with pytest.raises(ValueError, match="sums to 4"):
        la.mask_nms(a, s, counts=[2, 2])
    with pytest.raises(ValueError, match="need counts"):
        la.mask_nms(fa, np.zeros(6), frames=grid)
    with pytest.raises(ValueError, match="overlap must be"):
        la.mask_nms(a, s, overlap=(1, 2))
    with pytest.raises(ValueError, match="on the GPU"):
        la.mask_nms(a, s)


def test_the_restatement_on_cases_worked_by_hand():
    A = np.zeros((3, 4, 8), bool)
    A[0, :2] = True                  # 16 pixels
    A[1, 1:3, :4] = True             # 8 pixels, 4 of them in A[0]
    B = np.ones((1, 4, 8), bool)
    inter, aa, ab = MC.overlap_ref(A, B)
    assert inter.tolist() == [[16], [8], [0]] and aa.tolist() == [16, 8, 0] and ab.tolist() == [32]
    assert MC.ratio_ref(inter, aa, ab, "iou").tolist() == [[0.5], [0.25], [0.0]]
    assert MC.ratio_ref(inter, aa, ab, "iom").tolist() == [[1.0], [1.0], [0.0]]       # den == 0 gives 0.0
    assert MC.ratio_ref(inter, aa, ab, "ioa").tolist() == [[1.0], [1.0], [0.0]]
    self_i, a, _ = MC.overlap_ref(A, A)
    assert self_i.tolist() == [[16, 4, 0], [4, 8, 0], [0, 0, 0]]
    # iou(0, 1) = 4 / 20 = 0.2: suppressed below it, not at it (a strict comparison), never at 1.0; iom(0, 1) = 0.5
    assert MC.nms_ref(self_i, a, [0.9, 0.8, 0.7], 0.19).tolist() == [True, False, True]
    assert MC.nms_ref(self_i, a, [0.9, 0.8, 0.7], 0.2).tolist() == [True, True, True]
    assert MC.nms_ref(self_i, a, [0.9, 0.8, 0.7], 0.4, kind="iom").tolist() == [True, False, True]
    assert MC.nms_ref(self_i, a, [0.9, 0.8, 0.7], 0.19, labels=[1, 2, 1]).tolist() == [True, True, True]
    assert MC.nms_ref(self_i, a, [0.8, 0.8, np.nan], 0.0).tolist() == [True, False, False]   # a tie goes to the lower row; NaN is never kept
    assert MC.nms_ref(self_i, a, [np.nan, 0.8, 0.1], 0.0).tolist() == [False, True, True]    # and suppresses nothing
    m = MC.with_specials(MC.blobs(3, 7, 33, 47))
    assert m[0].all() and not m[1].any() and (m[2] == m[3]).all() and (m[5] <= m[4]).all() and m[5].sum() < m[4].sum()
