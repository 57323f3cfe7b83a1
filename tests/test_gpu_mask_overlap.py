"""GPU tests of mask overlap on bit planes (include/la3d.h "mask overlap on bit planes"): la3d_mask_overlap and la3d_mask_nms against
the NumPy restatement of tests/mask_overlap_cases.py.  Everything is compared EXACTLY: inter and the areas as integers, the ratios
bit for bit against NumPy's float64 division, keep as booleans."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from . import frames_fault_rows as FR
from . import mask_overlap_cases as MC
from . import open_bits_frames_cases as FC

pytestmark = pytest.mark.gpu

SENTINEL = -0x5a5a5a5b


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def np_(t):
    return t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()


def same_bits(got, want):
    """float64 arrays equal bit for bit (NaN patterns aside: NaN where and only where wanted)"""
    got, want = np_(got), np.asarray(want, np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all()
    assert (got[~nan].view(np.int64) == want[~nan].view(np.int64)).all()


def check(ov, ref, kind=None):
    inter, area_a, area_b, offsets, ratio = ref
    assert ov.inter.dtype.is_floating_point is False and np_(ov.inter).dtype == np.int32
    assert ov.offsets.tolist() == offsets.tolist() and ov.offsets.dtype == np.int64
    assert (np_(ov.inter) == inter).all()
    assert (np_(ov.area_a) == area_a).all() and (np_(ov.area_b) == area_b).all()
    if kind:
        same_bits(ov.iou, ratio)
    else:
        assert ov.iou is None


FRAMES = [(33, 47), (96, 224), (140, 96)]
PAIRS = [(1, 1), (7, 9), (8, 8), (9, 7), (17, 1), (1, 17), (17, 17), (8, 9)]


@pytest.fixture(scope="module")
def stacks():
    """17 + 17 masks per frame size and their 17 x 17 reference, computed once and left unchanged"""
    out = {}
    for k, (H, W) in enumerate(FRAMES):
        A = MC.with_specials(MC.blobs(100 + k, 17, H, W))
        B = MC.blobs(200 + k, 17, H, W)
        B[3], B[6], B[16] = A[2], True, False                              # an identical pair across the sides, all ones, empty
        out[(H, W)] = (A, B, MC.overlap_ref(A, B), MC.overlap_ref(A, A))
    return out


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("size", FRAMES)
def test_tile_edges_on_small_frames(la, stacks, size, pad):
    """na, nb in {1, 7, 8, 9, 17}: whole tiles, edge tiles, more than one tile per side; the unpadded 33 x 47 frame has 49-word
    planes at odd strides - the word-by-word path -, and so has every slice that starts at an odd row of it"""
    H, W = size
    A, B, (inter, aa, ab), (self_i, _, _) = stacks[size]
    a, b = la.pack_mask_bits(A, frame_pad=pad), la.pack_mask_bits(B, frame_pad=pad)
    if size == (33, 47) and not pad:
        assert a.bits.shape[1] == 49 and a.bits.stride(0) == 49
    for kind in (None, "iou", "iom", "ioa"):
        for na, nb in PAIRS if kind in (None, "iou") else PAIRS[1:2]:
            for s in (0, 17 - max(na, nb)):                               # the first rows, and the last ones (another base address)
                ov = la.mask_overlap(la.MaskBits(a.bits[s:s + na], *a[1:]), la.MaskBits(b.bits[s:s + nb], *b[1:]), iou=kind)
                i = inter[s:s + na, s:s + nb]
                ref = (i.reshape(-1), aa[s:s + na], ab[s:s + nb], np.array([0, na * nb]),
                       MC.ratio_ref(i, aa[s:s + na], ab[s:s + nb], kind).reshape(-1) if kind else None)
                check(ov, ref, kind)
                assert tuple(ov.matrix(0).shape) == (na, nb) and (np_(ov.matrix(0)) == i).all()
    for n in (1, 7, 8, 9, 17):                                            # the self form: symmetric, the areas on its diagonal
        ov = la.mask_iou(la.MaskBits(a.bits[:n], *a[1:]))
        m = np_(ov.matrix(0))
        assert (m == self_i[:n, :n]).all() and (m == m.T).all() and (np.diag(m) == aa[:n]).all()
        assert ov.area_a.data_ptr() == ov.area_b.data_ptr() and (np_(ov.area_a) == aa[:n]).all()
        same_bits(ov.matrix(0, "iou"), MC.ratio_ref(self_i[:n, :n], aa[:n], aa[:n], "iou"))
    ov = la.mask_overlap(a, iou="ioa")                                    # the one ratio that is not symmetric, mirrored
    same_bits(ov.matrix(0, "iou"), MC.ratio_ref(self_i, aa, aa, "ioa"))


def test_one_small_group_takes_the_word_split_path(la):
    """one 640 x 480 group of 3 x 3 rows, with the largest count of the frame (307 200) and an empty plane: the plan splits the words"""
    H, W = 480, 640
    A = MC.blobs(7, 3, H, W)
    B = MC.blobs(8, 3, H, W)
    A[0], A[1], B[2], B[0] = True, False, True, A[2]
    a, b = la.pack_mask_bits(A), la.pack_mask_bits(B)
    plan = la.mask_overlap_plan(a, b)
    t = plan.tiles_host
    assert len(t) == 10 and (t["nchunks"] == 10).all() and t["w1"].max() == 9600 and (t["ni"] == 3).all() and (t["nj"] == 3).all()
    ref = MC.groups_ref(A, B, [3], [3], "iou")
    assert ref[0].reshape(3, 3)[0, 2] == 307200 and ref[0].reshape(3, 3)[1].tolist() == [0, 0, 0]
    check(la.mask_overlap(a, b, iou="iou"), ref, "iou")
    check(la.mask_overlap(a, b, iou="iou", plan=plan), ref, "iou")
    ov = la.mask_overlap(a)
    assert len(la.mask_overlap_plan(a).tiles_host) == 10
    check(ov, MC.groups_ref(A, A, [3], [3]))


COUNTS_A = [0, 1, 9, 0, 17, 3, 8, 2, 0, 7, 1, 5]
COUNTS_B = [2, 0, 9, 0, 1, 17, 3, 8, 1, 0, 7, 4]


def test_ragged_groups(la):
    """12 images, groups that are empty on one side only (their areas are still written) and on both"""
    H, W = 33, 47
    A, B = MC.with_specials(MC.blobs(31, sum(COUNTS_A), H, W)), MC.blobs(32, sum(COUNTS_B), H, W)
    for pad in (True, False):
        a, b = la.pack_mask_bits(A, frame_pad=pad), la.pack_mask_bits(B, frame_pad=pad)
        for kind in (None, "iou", "ioa"):
            ref = MC.groups_ref(A, B, COUNTS_A, COUNTS_B, kind)
            assert ref[3].tolist() == np.concatenate([[0], np.cumsum(np.multiply(COUNTS_A, COUNTS_B))]).tolist()
            ov = la.mask_overlap(a, b, counts_a=COUNTS_A, counts_b=COUNTS_B, iou=kind)
            check(ov, ref, kind)
            for g in (2, 4, 5):
                ra, rb = sum(COUNTS_A[:g]), sum(COUNTS_B[:g])
                want = MC.overlap_ref(A[ra:ra + COUNTS_A[g]], B[rb:rb + COUNTS_B[g]])[0]
                assert tuple(ov.matrix(g).shape) == want.shape and (np_(ov.matrix(g)) == want).all()
            assert ov.matrix(0).shape == (0, 2) and ov.matrix(1).shape == (1, 0)
        ov = la.mask_overlap(a, counts_a=COUNTS_A, iou="iom")
        check(ov, MC.groups_ref(A, A, COUNTS_A, COUNTS_A, "iom"), "iom")
    empty = la.mask_overlap(la.MaskBits(a.bits[:0], *a[1:]), iou="iou")
    assert empty.inter.numel() == 0 and empty.iou.numel() == 0 and empty.offsets.tolist() == [0, 0]


def raw_call(la, a, b, plan, inter, area_a, area_b, iou, ws, kind):
    from labelany3d_amd import _lib

    import torch

    args = _lib.MaskOverlapArgs(struct_size=C.sizeof(_lib.MaskOverlapArgs), G=len(plan.counts_a), kind=kind, rows_a=a.bits.shape[0],
                                rows_b=b.bits.shape[0], a_bits=a.bits.data_ptr(), b_bits=b.bits.data_ptr(), a_stride=a.bits.stride(0),
                                b_stride=b.bits.stride(0), nwords=MC.plane_words(a.H, a.W), tiles=plan.tiles.data_ptr(),
                                ntiles=len(plan.tiles_host), npairs=int(plan.offsets[-1]), inter=inter.data_ptr(), area_a=area_a.data_ptr(),
                                area_b=area_b.data_ptr(), iou=iou.data_ptr(), workspace=ws.data_ptr(),
                                stream=torch.cuda.current_stream().cuda_stream)
    assert _lib.lib.la3d_mask_overlap(C.byref(args)) == 0, _lib.lib.la3d_last_error()


@pytest.mark.parametrize("stride", [68, 67])
def test_every_output_is_written_and_nothing_else(la, stride):
    """the caller's buffers hold a sentinel and the planes' buffer is over-allocated (sentinel words between the planes): every element
    below offsets[G] is written, nothing beyond it is, and nothing depends on what the workspace held.  A 33 x 64 plane has 66 words:
    at stride 68 the 16-byte path ends in a part of a group, at stride 67 the planes are read word by word"""
    import torch

    H, W = 33, 47
    ca, cb = [9, 0, 8, 3], [7, 2, 17, 0]
    A, B = MC.with_specials(MC.blobs(41, sum(ca), H, W)), MC.blobs(42, sum(cb), H, W)
    dev = torch.device("cuda", 0)
    bufs = [torch.full((n, stride), SENTINEL, dtype=torch.int32, device=dev) for n in (sum(ca), sum(cb))]
    a, b = la.pack_mask_bits(A, out=bufs[0]), la.pack_mask_bits(B, out=bufs[1])
    assert a.bits.stride(0) == stride and (np_(bufs[0])[:, 66:] == SENTINEL).all()
    plan = la.mask_overlap_plan(a, b, ca, cb)
    npairs, extra = int(plan.offsets[-1]), 64
    ref = MC.groups_ref(A, B, ca, cb, "iou")
    for fill in (SENTINEL, 0x12345678):
        inter = torch.full((npairs + extra,), SENTINEL, dtype=torch.int32, device=dev)
        area_a = torch.full((sum(ca) + extra,), SENTINEL, dtype=torch.int32, device=dev)
        area_b = torch.full((sum(cb) + extra,), SENTINEL, dtype=torch.int32, device=dev)
        iou = torch.full((npairs + extra,), -7.0, dtype=torch.float64, device=dev)
        plan.workspace.fill_(fill)
        raw_call(la, a, b, plan, inter, area_a, area_b, iou, plan.workspace, 1)
        torch.cuda.synchronize()
        assert (np_(inter)[:npairs] == ref[0]).all() and (np_(inter)[npairs:] == SENTINEL).all()
        assert (np_(area_a)[:sum(ca)] == ref[1]).all() and (np_(area_a)[sum(ca):] == SENTINEL).all()
        assert (np_(area_b)[:sum(cb)] == ref[2]).all() and (np_(area_b)[sum(cb):] == SENTINEL).all()
        same_bits(iou[:npairs], ref[4])
        assert (np_(iou)[npairs:] == -7.0).all()
    assert (np_(bufs[0])[:, 66:] == SENTINEL).all() and (np_(bufs[1])[:, 66:] == SENTINEL).all()


SIZES = [(33, 47), (96, 224), (140, 96)]
F_A, F_B = [9, 3, 17], [8, 0, 9]


def test_frames_form_equals_the_uniform_calls_and_refuses_bad_rows(la):
    import torch

    A = [MC.with_specials(MC.blobs(51 + p, F_A[p], h, w)) for p, (h, w) in enumerate(SIZES)]
    B = [MC.blobs(61 + p, F_B[p], h, w) for p, (h, w) in enumerate(SIZES)]
    pa, pb = la.pack_mask_frames(A), la.pack_mask_frames(B)
    fa, fb = la.pack_mask_bits_frames(pa), la.pack_mask_bits_frames(pb)
    ov = la.mask_overlap(fa, fb, counts_a=F_A, counts_b=F_B, frames=pa, iou="iou")
    self_ov = la.mask_overlap(fa, counts_a=F_A, frames=pa, iou="iom")
    for p in range(3):
        one = la.mask_overlap(la.pack_mask_bits(A[p]), la.pack_mask_bits(B[p]), iou="iou")
        ref = MC.groups_ref(A[p], B[p], [F_A[p]], [F_B[p]], "iou")
        check(one, ref, "iou")
        assert (np_(ov.matrix(p)) == np_(one.matrix(0))).all()
        same_bits(ov.matrix(p, "iou"), np_(one.matrix(0, "iou")))
        ra, rb = sum(F_A[:p]), sum(F_B[:p])
        assert (np_(ov.area_a)[ra:ra + F_A[p]] == ref[1]).all() and (np_(ov.area_b)[rb:rb + F_B[p]] == ref[2]).all()
        sref = MC.groups_ref(A[p], A[p], [F_A[p]], [F_A[p]], "iom")
        assert (np_(self_ov.matrix(p)).reshape(-1) == sref[0]).all()
        same_bits(self_ov.matrix(p, "iou").reshape(-1), sref[4])
    # one row with another image's index, one whose offset is not a multiple of 4 - both in bounds, so nothing can fault -, and one
    # whose plane would end beyond the buffer: refused on the device, every other pair unchanged
    ii, offs = fa.image_index.clone(), fa.offsets.clone()
    ii[2] = 1
    offs[10] += 2
    offs[20] = fa.bits.numel() - 8
    bad = fa._replace(image_index=ii, offsets=offs)
    refused = [2, 10, 20]
    got = la.mask_overlap(bad, fb, counts_a=F_A, counts_b=F_B, frames=pa, iou="iou")
    want_i, want_r, want_a = np_(ov.inter).copy(), np_(ov.iou).copy(), np_(ov.area_a).copy()
    rows = np.concatenate([np.repeat(np.arange(sum(F_A[:p]), sum(F_A[:p + 1])), F_B[p]) for p in range(3)])   # the row of A of each pair
    hit = np.isin(rows, refused)
    want_i[hit], want_r[hit], want_a[refused] = -1, np.nan, -1
    assert hit.sum() == 8 + 0 + 9
    assert (np_(got.inter) == want_i).all() and (np_(got.area_a) == want_a).all() and (np_(got.area_b) == np_(ov.area_b)).all()
    same_bits(got.iou, want_r)
    sgot = la.mask_overlap(bad, counts_a=F_A, frames=pa)                    # the self form: the row's row AND column
    for p in range(3):
        m, w = np_(sgot.matrix(p)), np_(self_ov.matrix(p)).copy()
        for r in refused:
            k = r - sum(F_A[:p])
            if 0 <= k < F_A[p]:
                w[k, :], w[:, k] = -1, -1
        assert (m == w).all()
    assert (np_(sgot.area_a)[refused] == -1).all()
    # NMS never keeps a refused row, and it suppresses nothing
    keep = np_(la.mask_nms(bad, np.arange(29, 0, -1.0), iou_threshold=0.0, counts=F_A, frames=pa))
    ok = np_(la.mask_nms(fa, np.arange(29, 0, -1.0), iou_threshold=0.0, counts=F_A, frames=pa))
    assert not keep[refused].any() and keep[0] and ok[0]
    for p in range(3):
        r0 = sum(F_A[:p])
        m = np_(sgot.matrix(p))
        assert (keep[r0:r0 + F_A[p]] == MC.nms_ref(m, np_(sgot.area_a)[r0:r0 + F_A[p]], np.arange(29, 0, -1.0)[r0:r0 + F_A[p]], 0.0)).all()
    torch.cuda.synchronize()
    frames_fault_rows(la)


def frames_fault_rows(la):
    """The shared case table (tests/frames_fault_rows.py), one fault per row, in the group-keyed form of this entry: group g is image g
    of the table, so a frame row that breaks the contract refuses its whole group, and an image index that is not the group's (-1, P)
    refuses its row.  The table and the planes have pad in front and behind: a defect shows as a count that is not -1, never as a
    fault."""
    import torch

    good, P, SLOT, PAD = FR.GOOD, FR.P, FR.SLOT, FR.PAD
    bad_groups = [(3 + j, name) for j, (name, _) in enumerate(FR.FRAME_FAULTS)]
    #         image  what                                   (the rows of a group are contiguous; each good group begins and ends well)
    rows_a = [(0, None), (-1, FR.INDEX_FAULTS[0]), (0, FR.END_FAULT), (0, None),
              (1, None), (P, FR.INDEX_FAULTS[1]), (1, FR.OFFSET_FAULTS[1]), (1, None),
              (2, None), (2, FR.OFFSET_FAULTS[0]), (2, None)] + bad_groups
    rows_b = [(0, None), (0, None), (1, None), (1, None), (2, None), (2, None)] + bad_groups
    ca, cb = [4, 4, 3] + [1] * len(bad_groups), [2, 2, 2] + [1] * len(bad_groups)
    group_a = np.repeat(np.arange(P), ca)                                   # the group a row stands in, whatever its image index says
    rs = np.random.RandomState(8)

    def side(rows):
        c = SimpleNamespace(rows=rows, B=len(rows), P=P, H=FR.H, W=FR.W, words=len(rows) * SLOT + 1, table=FR.frame_table(),
                            offsets=np.arange(len(rows), dtype=np.int64) * SLOT, image_index=np.array([img for img, _ in rows], np.int32),
                            good=[n for n, (img, bad) in enumerate(rows) if bad is None])
        for n, (img, bad) in enumerate(rows):
            if bad == FR.OFFSET_FAULTS[0]:
                c.offsets[n] = -4
            elif bad == FR.OFFSET_FAULTS[1]:
                c.offsets[n] += 2
            elif bad == FR.END_FAULT:
                c.offsets[n] = c.words - FR.plane_words(*good[img]) + 1
                assert c.offsets[n] % 4 == 0 and c.offsets[n] >= 0
        masks = {n: MC.blobs(int(rs.randint(1 << 30)), 1, *good[rows[n][0]])[0] for n in c.good}
        inbuf = FR.input_words(c, rs, lambda n, h, w: FC.frame_words(masks[n]))
        return c, masks, inbuf, FR.on_device(c, inbuf)

    (A, ma, buf_a, da), (B, mb, buf_b, db) = side(rows_a), side(rows_b)
    grid = FR.frame_grid(la, A, da)
    got = la.mask_overlap(FR.frame_bits(la, A, da), FR.frame_bits(la, B, db), counts_a=ca, counts_b=cb, frames=grid, iou="iou")
    # the call without the bad rows: the good rows of the good groups only
    ga = [[n for n in A.good if group_a[n] == g] for g in range(3)]
    gb = [[n for n in B.good if rows_b[n][0] == g] for g in range(3)]
    zeros = [0] * len(bad_groups)
    ref = la.mask_overlap(FR.frame_bits(la, A, da, sum(ga, [])), FR.frame_bits(la, B, db, sum(gb, [])), counts_a=[len(x) for x in ga] + zeros,
                          counts_b=[len(x) for x in gb] + zeros, frames=grid, iou="iou")
    assert int(np_(ref.inter).sum()) > 0
    area_a, area_b = np_(got.area_a), np_(got.area_b)
    first_a = np.concatenate([[0], np.cumsum(ca)])
    for g in range(P):
        m, r = np_(got.matrix(g)), np_(got.matrix(g, "iou"))
        if g >= 3:                                                            # a frame row that breaks the contract: the whole group
            assert (m == -1).all() and np.isnan(r).all() and m.shape == (1, 1), (g, rows_a[first_a[g]][1])
            assert area_a[first_a[g]] == -1 and area_b[6 + g - 3] == -1, g
            continue
        want, want_r = np_(ref.matrix(g)), np_(ref.matrix(g, "iou"))
        k = 0
        for i in range(ca[g]):
            n = first_a[g] + i
            if rows_a[n][1] is None:
                assert (m[i] == want[k]).all() and area_a[n] == ma[n].sum(), (n, g)
                same_bits(r[i], want_r[k])
                k += 1
            else:
                assert (m[i] == -1).all() and np.isnan(r[i]).all() and area_a[n] == -1, (n, rows_a[n][1])
        assert k == len(ga[g]) and (area_b[2 * g:2 * g + 2] == [mb[n].sum() for n in gb[g]]).all()
    assert {bad for _, bad in rows_a} >= set(FR.INDEX_FAULTS + FR.OFFSET_FAULTS + [FR.END_FAULT] + [f for f, _ in FR.FRAME_FAULTS])
    np.testing.assert_array_equal(np_(da.bits_all).view(np.uint32), buf_a)
    np.testing.assert_array_equal(np_(db.bits_all).view(np.uint32), buf_b)


def test_the_source_of_the_planes_does_not_matter(la):
    import torch

    H, W = 33, 47
    A = MC.with_specials(MC.blobs(71, 9, H, W))
    want = MC.groups_ref(A, A, [9], [9], "iou")
    logits = torch.as_tensor(np.where(A, 1.5, -0.5).astype(np.float32), device="cuda")
    rles = [{"size": [H, W], "counts": MC.rle_counts(m)} for m in A]
    for pad in (True, False):
        for mb in (la.pack_mask_bits(A, frame_pad=pad), la.pack_rle_bits(rles, frame_pad=pad), la.pack_logits_bits(logits, frame_pad=pad)):
            check(la.mask_overlap(mb, iou="iou"), want, "iou")


def nms_case(la, masks, scores, thr, counts=None, labels=None, kind="iou", pad=True):
    counts = [len(masks)] if counts is None else counts
    mb = la.pack_mask_bits(masks, frame_pad=pad)
    got = np_(la.mask_nms(mb, scores, iou_threshold=thr, counts=None if len(counts) == 1 else counts, labels=labels, kind=kind))
    assert got.dtype == np.bool_ and got.shape == (len(masks),)
    r0 = 0
    for n in counts:
        inter, area, _ = MC.overlap_ref(masks[r0:r0 + n], masks[r0:r0 + n])
        want = MC.nms_ref(inter, area, np.asarray(scores)[r0:r0 + n], thr, None if labels is None else np.asarray(labels)[r0:r0 + n], kind)
        assert (got[r0:r0 + n] == want).all(), (r0, n, thr, kind)
        r0 += n
    return got


def strips(H, W, spans):
    m = np.zeros((len(spans), H, W), bool)
    for i, (c0, c1) in enumerate(spans):
        m[i, :, c0:c1] = True
    return m


def test_nms_duplicates_nested_masks_and_chains(la):
    H, W = 32, 96
    # a chain: iou(a, b) = iou(b, c) = 25 / 55, iou(a, c) = 10 / 70 - a suppresses b, b would have suppressed c, c survives
    chain = strips(H, W, [(0, 40), (15, 55), (30, 70)])
    assert nms_case(la, chain, [0.9, 0.8, 0.7], 0.3).tolist() == [True, False, True]
    assert nms_case(la, chain, [0.7, 0.9, 0.8], 0.3).tolist() == [False, True, False]
    # duplicates and a nested mask: iou(big, small) = 1 / 4, iom = 1
    m = strips(H, W, [(0, 80), (0, 80), (20, 40), (90, 96)])
    assert nms_case(la, m, [0.5, 0.6, 0.9, 0.1], 0.5).tolist() == [False, True, True, True]
    assert nms_case(la, m, [0.5, 0.6, 0.9, 0.1], 0.5, kind="iom").tolist() == [False, False, True, True]
    assert nms_case(la, m, [0.5, 0.6, 0.4, 0.1], 0.5, kind="iom").tolist() == [False, True, False, True]
    # tied scores go to the lower row; a NaN score is never kept and suppresses nothing
    assert nms_case(la, m, [0.5, 0.5, 0.5, 0.5], 0.5).tolist() == [True, False, True, True]
    assert nms_case(la, m, [np.nan, 0.5, 0.9, 0.1], 0.5).tolist() == [False, True, True, True]
    assert nms_case(la, m, [0.9, np.nan, 0.8, np.nan], 0.2).tolist() == [True, False, False, False]
    # labels keep two identical masks of different classes
    assert nms_case(la, m, [0.5, 0.6, 0.9, 0.1], 0.5, labels=[1, 2, 1, 1]).tolist() == [True, True, True, True]
    assert nms_case(la, m, [0.5, 0.6, 0.9, 0.1], 0.5, labels=[3, 3, 1, 1]).tolist() == [False, True, True, True]
    # the thresholds' ends: 0.0 suppresses whatever touches, 1.0 nothing - not even a duplicate (a strict comparison)
    assert nms_case(la, m, [0.5, 0.6, 0.9, 0.1], 0.0).tolist() == [False, False, True, True]
    assert nms_case(la, m, [0.5, 0.6, 0.9, 0.1], 1.0).tolist() == [True, True, True, True]
    # an empty plane has den 0 against itself: it is kept and suppresses nothing
    e = strips(H, W, [(0, 0), (0, 0), (0, 10)])
    assert nms_case(la, e, [0.9, 0.8, 0.7], 0.0).tolist() == [True, True, True]


def test_nms_over_several_groups_against_the_plain_loop(la):
    """several groups at once, 70 rows in one of them (the visiting loop goes past a wave), random blobs with duplicates, tied and NaN
    scores, labels; device scores and host scores; overlap= given and not given agree"""
    import torch

    H, W = 33, 47
    counts = [5, 0, 70, 1, 24]
    n = sum(counts)
    rs = np.random.RandomState(5)
    masks = MC.blobs(81, n, H, W)
    masks[10], masks[40], masks[76] = masks[7], masks[39], False
    scores = np.round(rs.rand(n), 2)                                      # two decimals: ties
    scores[[3, 20, 77]] = np.nan
    labels = rs.randint(0, 3, n)
    for thr in (0.0, 0.3, 0.5, 1.0):
        for kind in ("iou", "iom"):
            for lab in (None, labels):
                a = nms_case(la, masks, scores, thr, counts, lab, kind, pad=False)
        assert 0 < a.sum() <= n
    mb = la.pack_mask_bits(masks)
    ov = la.mask_overlap(mb, counts_a=counts, iou="iou")
    dev_scores = torch.as_tensor(scores.astype(np.float32), device="cuda")
    for kind in ("iou", "iom"):
        want = np_(la.mask_nms(mb, scores.astype(np.float32), 0.5, counts=counts, labels=labels, kind=kind))
        assert (np_(la.mask_nms(mb, dev_scores, 0.5, counts=counts, labels=torch.as_tensor(labels, device="cuda"), kind=kind, overlap=ov)) == want).all()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = la.mask_nms(mb, dev_scores, 0.5, counts=counts, labels=labels, kind="iom", stream=side)
    side.synchronize()
    assert (np_(got) == want).all()
    assert la.mask_nms(la.MaskBits(mb.bits[:0], *mb[1:]), np.zeros(0)).shape == (0,)


def test_one_captured_call_replays_on_new_planes(la):
    """tables and workspace prepared beforehand: the call is two kernel launches - captured on a side stream, replayed on new contents"""
    import torch

    H, W = 96, 224
    ca, cb = [9, 3, 0], [8, 5, 2]
    sets = [(MC.blobs(91 + k, sum(ca), H, W), MC.blobs(95 + k, sum(cb), H, W)) for k in range(2)]
    a, b = la.pack_mask_bits(sets[0][0]), la.pack_mask_bits(sets[0][1])
    plan = la.mask_overlap_plan(a, b, ca, cb)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        la.mask_overlap(a, b, ca, cb, iou="iou", plan=plan, stream=side)   # (warm-up)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            ov = la.mask_overlap(a, b, ca, cb, iou="iou", plan=plan, stream=torch.cuda.current_stream())
    for k in (1, 0):
        a.bits.copy_(la.pack_mask_bits(sets[k][0]).bits)
        b.bits.copy_(la.pack_mask_bits(sets[k][1]).bits)
        ov.inter.fill_(SENTINEL)
        ov.iou.fill_(-7.0)
        plan.workspace.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(ov, MC.groups_ref(sets[k][0], sets[k][1], ca, cb, "iou"), "iou")
        check(la.mask_overlap(a, b, ca, cb, iou="iou"), MC.groups_ref(sets[k][0], sets[k][1], ca, cb, "iou"), "iou")
