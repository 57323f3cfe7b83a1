"""GPU tests of morphology on bit planes (include/la3d.h "morphology on bit planes"; ``open_bits``, ``bits_rects``, ``select_crops``):
the opened planes against what SciPy gave (tests/golden/g19_opening.npz) and against the NumPy restatement of the rule
(tests/open_bits_cases.py), bit for bit on the plane words and exact on the statistics; squares and bars across every band seam; the
smallest frames and the widths around a word; plane strides, ``out`` reuse and the statistics-only call; the algebra of an opening;
the consumers of the planes; the crop stage's gate; one captured call."""
import numpy as np
import pytest

from . import instance_points_cases as IC
from . import open_bits_cases as OC

pytestmark = pytest.mark.gpu

SENTINEL = OC.SENTINEL


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


@pytest.fixture(scope="module")
def g():
    return OC.load_golden()


def np_(t):
    return t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()


def u32(t):
    return np_(t).view(np.uint32)


def planes_of(la, masks, pad=True):
    import torch

    return la.pack_mask_bits(torch.as_tensor(np.ascontiguousarray(masks).astype(np.uint8), device="cuda"), frame_pad=pad)


def check_planes(mb, stats, want, H, W, W_out, tag):
    """mb: the opened MaskBits; want: the expected (H, W) bool masks"""
    assert (mb.H, mb.W, mb.frame_width) == (H, W_out, W), (tag, mb.H, mb.W, mb.frame_width)
    got = u32(mb.bits)
    nwords = (H * W_out + 31) // 32
    assert got.shape[0] == len(want) and got.shape[1] >= nwords, tag
    for b, m in enumerate(want):
        assert m.shape == (H, W), tag
        np.testing.assert_array_equal(got[b, :nwords], OC.words(m, W_out), err_msg=f"{tag}[{b}]")
    if stats is not None:
        assert stats.dtype.is_floating_point is False and tuple(stats.shape) == (len(want), 5), tag
        np.testing.assert_array_equal(np_(stats), np.array([OC.rect_stats(m) for m in want], np.int32).reshape(len(want), 5), err_msg=f"{tag} stats")


def opened_all(masks, k, s):
    return [OC.opening(m, k, s) for m in masks]


# ------------------------------------------------------------------------------------------
# 1. the fixture: SciPy's planes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,pad_in,pad_out", [(0, False, False), (0, True, True), (0, False, True), (0, True, False), (1, True, True),
                                              (1, False, False), (2, True, True), (2, False, False)],
                         ids=["33x47", "33x47pp", "33x47-p", "33x47p-", "96x224pp", "96x224", "140x96pp", "140x96"])
def test_fixture_planes_bit_for_bit(la, g, f, pad_in, pad_out):
    """every k and factor of the frame, rows padded and unpadded on either side: SciPy's own planes, and the rectangles of them"""
    H, W = OC.FRAMES[f]
    seen = 0
    for i, (fi, k, s) in enumerate(OC.fixture_cases()):
        if fi != f:
            continue
        ins, outs = OC.golden_case(g, i)
        mb, stats = la.open_bits(planes_of(la, ins, pad_in), k=k, upscale=s, frame_pad=pad_out, return_stats=True)
        check_planes(mb, stats, list(outs), s * H, s * W, OC.padded(s * W) if pad_out else s * W, f"fixture {H}x{W} k={k} s={s}")
        seen += 1
    assert seen == 9


# ------------------------------------------------------------------------------------------
# 2. band seams
# ------------------------------------------------------------------------------------------
def seam_batch(H, W, side_h, side_w, x0):
    """one plane per offset: a side_h x side_w block of source pixels with its top row at every offset 0 .. H - side_h"""
    tops = range(0, H - side_h + 1)
    m = np.zeros((len(tops), H, W), bool)
    for n, t in enumerate(tops):
        m[n, t:t + side_h, x0:x0 + side_w] = True
    return m


@pytest.mark.parametrize("H,W,s,x0", [(140, 96, 1, 41), (40, 64, 4, 9), (140, 65, 1, 58)], ids=["140x96s1", "40x64s4", "140x65s1-right-edge"])
def test_squares_survive_and_bars_vanish_at_every_row_offset(la, H, W, s, x0):
    """k = 7.  At s = 1 a k x k square with its top row at every offset 0 .. H_out - k comes back unchanged and a (k - 1) x k bar vanishes,
    whatever band seam it straddles.  At s = 4 an upscaled block has sides that are multiples of 4, so the square is the smallest
    source block that survives - 2 x 2 source pixels, 8 x 8 after the upscale - at every SOURCE row offset (every fourth output row: the
    band seams are multiples of 32, so each is straddled), and the bar is one source row high (4 < k output rows) and 2 wide."""
    k = 7
    sq = k if s == 1 else 2
    squares = seam_batch(H, W, sq, sq, x0)
    bars = seam_batch(H, W, k - 1 if s == 1 else 1, sq, x0)
    assert len(squares) == H - sq + 1 and s * sq >= k
    for pad in (True, False):
        mb, stats = la.open_bits(planes_of(la, squares, pad), k=k, upscale=s, frame_pad=pad, return_stats=True)
        want = [OC.upscale(m, s) for m in squares]
        check_planes(mb, stats, want, s * H, s * W, OC.padded(s * W) if pad else s * W, f"squares pad={pad}")
        st = np_(stats)
        assert (st[:, 0] == (s * sq) ** 2).all() and (st[:, 2] == s * np.arange(len(squares))).all() and (st[:, 1] == s * x0).all()
        mb, stats = la.open_bits(planes_of(la, bars, pad), k=k, upscale=s, frame_pad=pad, return_stats=True)
        assert not u32(mb.bits).any() and not np_(stats).any(), f"bars pad={pad}"
    np.testing.assert_array_equal(np.stack(opened_all(squares[::17], k, s)), np.stack([OC.upscale(m, s) for m in squares[::17]]))


# ------------------------------------------------------------------------------------------
# 3. edges
# ------------------------------------------------------------------------------------------
def test_smallest_frames(la):
    for H, W, want_full in ((1, 1, False), (3, 3, False), (7, 7, True), (6, 9, False)):
        full = np.ones((1, H, W), bool)
        for pad in (False, True):
            mb, stats = la.open_bits(planes_of(la, full, pad), k=7, frame_pad=pad, return_stats=True)
            want = [np.full((H, W), want_full)]
            np.testing.assert_array_equal(OC.opening(full[0], 7), want[0])
            check_planes(mb, stats, want, H, W, OC.padded(W) if pad else W, f"full {H}x{W} pad={pad}")
    # the 7 x 7 frame at every factor: 1 x 1 .. 3 x 3 source pixels never reach 7 at s = 1, 2; a 2 x 2 frame does at s = 4
    for s, want_full in ((1, False), (2, False), (4, True)):
        mb, stats = la.open_bits(planes_of(la, np.ones((1, 2, 2), bool), False), k=7, upscale=s, frame_pad=False, return_stats=True)
        check_planes(mb, stats, [np.full((2 * s, 2 * s), want_full)], 2 * s, 2 * s, 2 * s, f"2x2 s={s}")


@pytest.mark.parametrize("W", [31, 32, 33, 64, 65])
def test_widths_around_a_word(la, W):
    rs = np.random.RandomState(W)
    H = 37
    masks = np.stack([OC.blob_plane(rs, H, W, noise=0.03) for _ in range(6)])
    for k, s, pad_in, pad_out in ((3, 1, False, False), (7, 2, True, False), (5, 4, False, True), (7, 1, True, True), (3, 4, False, False)):
        mb, stats = la.open_bits(planes_of(la, masks, pad_in), k=k, upscale=s, frame_pad=pad_out, return_stats=True)
        check_planes(mb, stats, opened_all(masks, k, s), s * H, s * W, OC.padded(s * W) if pad_out else s * W, f"W={W} k={k} s={s}")


def test_k1_is_the_identity_and_k31_runs(la, g):
    H, W = OC.FRAMES[1]
    rs = np.random.RandomState(31)
    masks = np.stack([OC.blob_plane(rs, H, W) for _ in range(3)] + [np.ones((H, W), bool)])
    masks[2, 20:70, 100:160] = True                       # a block that holds a 31 x 31 square
    for s in (1, 2, 4):
        mb, stats = la.open_bits(planes_of(la, masks), k=1, upscale=s, return_stats=True)
        check_planes(mb, stats, [OC.upscale(m, s) for m in masks], s * H, s * W, s * W, f"k=1 s={s}")
        mb, stats = la.open_bits(planes_of(la, masks), k=31, upscale=s, return_stats=True)
        want = opened_all(masks, 31, s)
        check_planes(mb, stats, want, s * H, s * W, s * W, f"k=31 s={s}")
        assert want[2].any() and want[3].all()
    np.testing.assert_array_equal(np_(la.bits_rects(planes_of(la, masks))), [OC.rect_stats(m) for m in masks])
    m47 = np.stack([OC.blob_plane(rs, 33, 47) for _ in range(3)])
    for pad in (False, True):
        np.testing.assert_array_equal(np_(la.bits_rects(planes_of(la, m47, pad))), [OC.rect_stats(m) for m in m47])


def test_garbage_past_the_plane_is_ignored(la):
    """H * W = 5 * 33 = 165 bits: the last word has 27 bits that are no pixels; set, they change nothing - nor does a stored width
    beyond the image when its columns hold what the format says (zeros) and the tail does not"""
    import torch

    H, W = 5, 33
    rs = np.random.RandomState(3)
    masks = rs.rand(4, H, W) < 0.8
    clean = planes_of(la, masks, False)
    dirty = clean.bits.clone()
    dirty[:, -1] |= torch.tensor(np.array([(0xFFFFFFFF << (H * W % 32)) & 0xFFFFFFFF], np.uint32).view(np.int32)[0], device="cuda")
    assert (u32(dirty)[:, -1] >> (H * W % 32) == (1 << (32 - H * W % 32)) - 1).all()
    for k, s in ((3, 1), (3, 2), (5, 4), (1, 1)):
        mb, stats = la.open_bits(la.MaskBits(dirty, H, W, W), k=k, upscale=s, frame_pad=False, return_stats=True)
        check_planes(mb, stats, opened_all(masks, k, s), s * H, s * W, s * W, f"dirty k={k} s={s}")
    np.testing.assert_array_equal(np_(la.bits_rects(la.MaskBits(dirty, H, W, W))), [OC.rect_stats(m) for m in masks])


# ------------------------------------------------------------------------------------------
# 4. layout
# ------------------------------------------------------------------------------------------
def test_long_strides_leave_the_words_between_planes_alone(la):
    import torch

    H, W, B = 33, 47, 5
    rs = np.random.RandomState(8)
    masks = np.stack([OC.blob_plane(rs, H, W) for _ in range(B)])
    for pad_in, pad_out, k, s in ((False, False, 3, 2), (True, True, 7, 4), (False, True, 3, 1)):
        src = planes_of(la, masks, pad_in)
        n_in = (H * src.W + 31) // 32
        big_in = torch.full((B, n_in + 3), SENTINEL, dtype=torch.int32, device="cuda")
        big_in[:, :n_in] = src.bits[:, :n_in]
        W_out = OC.padded(s * W) if pad_out else s * W
        n_out = (s * H * W_out + 31) // 32
        big_out = torch.full((B, n_out + 5), SENTINEL, dtype=torch.int32, device="cuda")
        before = u32(big_in).copy()
        mb, stats = la.open_bits(la.MaskBits(big_in[:, :n_in], H, src.W, W), k=k, upscale=s, frame_pad=pad_out, out=big_out[:, :n_out],
                                 return_stats=True)
        assert mb.bits.data_ptr() == big_out.data_ptr()
        check_planes(mb, stats, opened_all(masks, k, s), s * H, s * W, W_out, f"strides k={k} s={s}")
        assert (u32(big_out)[:, n_out:] == SENTINEL).all() and (u32(big_in) == before).all()


def test_out_reuse_and_calls_without_statistics_or_planes(la):
    import ctypes as C

    import torch

    from labelany3d_amd import _lib

    H, W, B, k, s = 33, 47, 6, 3, 2
    rs = np.random.RandomState(12)
    a, b = (np.stack([OC.blob_plane(rs, H, W) for _ in range(B)]) for _ in range(2))
    W_out = OC.padded(s * W)
    out = torch.full((B, (s * H * W_out + 31) // 32), SENTINEL, dtype=torch.int32, device="cuda")
    for masks in (a, b, a):
        mb = la.open_bits(planes_of(la, masks), k=k, upscale=s, out=out)             # stats=None
        assert isinstance(mb, la.MaskBits) and mb.bits is out
        check_planes(mb, None, opened_all(masks, k, s), s * H, s * W, W_out, "out reuse")
    # out_bits = NULL: the same statistics as the full call, nothing else written
    src = planes_of(la, a, False)
    _, full = la.open_bits(src, k=k, upscale=s, return_stats=True)
    stats = torch.full((B, 5), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(_lib.lib.la3d_open_bits_workspace_bytes(B, H, s) // 4, dtype=torch.int32, device="cuda")
    rc = _lib.lib.la3d_open_bits(C.c_void_p(src.bits.data_ptr()), src.bits.stride(0), B, H, src.W, W, k, s, None, 0, 0,
                                 C.c_void_p(stats.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib.la3d_last_error()
    np.testing.assert_array_equal(np_(stats), np_(full))
    np.testing.assert_array_equal(np_(full), [OC.rect_stats(m) for m in opened_all(a, k, s)])


@pytest.mark.parametrize("B", [0, 1, 300])
def test_batch_sizes(la, B):
    H, W = 40, 50
    rs = np.random.RandomState(B)
    base = np.stack([OC.blob_plane(rs, H, W) for _ in range(5)])
    masks = base[np.arange(B) % 5] if B else np.zeros((0, H, W), bool)
    if B:
        masks = masks.copy()
        masks[np.arange(B), np.arange(B) % H, :] ^= True        # no two planes alike
    mb, stats = la.open_bits(planes_of(la, masks, False), k=5, upscale=2, return_stats=True)
    check_planes(mb, stats, opened_all(masks, 5, 2), 2 * H, 2 * W, OC.padded(2 * W), f"B={B}")
    assert tuple(la.bits_rects(planes_of(la, masks)).shape) == (B, 5)


# ------------------------------------------------------------------------------------------
# 5. algebra
# ------------------------------------------------------------------------------------------
def test_an_opening_shrinks_and_is_idempotent(la):
    rs = np.random.RandomState(77)
    H, W = 70, 100
    masks = rs.rand(8, H, W) < np.array([0.5, 0.9, 0.9, 0.97, 0.97, 0.995, 0.995, 1.0])[:, None, None]
    for k, s in ((3, 1), (5, 2), (7, 4), (9, 1)):
        mb = la.open_bits(planes_of(la, masks, False), k=k, upscale=s)
        got = np_(la.unpack_mask_bits(mb))
        up = np.stack([OC.upscale(m, s) for m in masks])
        assert got.shape == up.shape and not (got & ~up).any(), (k, s)
        again = la.open_bits(mb, k=k, upscale=1, frame_pad=mb.W != mb.frame_width)
        assert (again.H, again.W, again.frame_width) == (mb.H, mb.W, mb.frame_width)
        np.testing.assert_array_equal(u32(again.bits), u32(mb.bits), err_msg=f"idempotent k={k} s={s}")
        assert got.any() and (got != up).any()


# ------------------------------------------------------------------------------------------
# 6. consumers
# ------------------------------------------------------------------------------------------
def test_consumers_take_the_opened_planes(la):
    H, W, B = 96, 224, 6
    rs = np.random.RandomState(21)
    masks = np.stack([OC.blob_plane(rs, H, W) for _ in range(B)])
    want = np.stack(opened_all(masks, 7, 1))
    assert want.any(axis=(1, 2)).sum() >= 4
    mb, stats = la.open_bits(planes_of(la, masks), k=7, return_stats=True)
    np.testing.assert_array_equal(np_(la.mask_stats_bits(mb))[:, 0], np_(stats)[:, 0])
    np.testing.assert_array_equal(np_(la.rle_decode(la.rle_encode_bits(mb))).astype(bool), want)
    depth, K = IC.special_depth(B, H, W), IC.cameras(B, H, W)
    got = la.fit_instances_bits(depth, mb, K)
    ref = la.fit_instances_bits(depth, planes_of(la, want), K)
    np.testing.assert_array_equal(np_(got[1]), np_(ref[1]))
    np.testing.assert_array_equal(np_(got[0]), np_(ref[0]))                     # (NaN == NaN in the same place)
    assert np.isfinite(np_(ref[0])).any()
    # an upscaled plane feeds them too
    mb4, st4 = la.open_bits(planes_of(la, masks[:2]), k=7, upscale=4, return_stats=True)
    np.testing.assert_array_equal(np_(la.mask_stats_bits(mb4))[:, 0], np_(st4)[:, 0])
    np.testing.assert_array_equal(np_(la.rle_decode(la.rle_encode_bits(mb4))).astype(bool), np.stack(opened_all(masks[:2], 7, 4)))


# ------------------------------------------------------------------------------------------
# 7. the crop stage's gate
# ------------------------------------------------------------------------------------------
def test_select_crops_is_the_reference_gate(la):
    """The reference's defaults (x4, 7 x 7, 6400 pixels, 512-pixel crops) on 120 x 160 sources.  After the x4 upscale every edge of a
    shape lies on a multiple of 4, so do the edges of every rectangle inscribed in it, and an opening by a square is the union of the
    inscribed rectangles whose sides reach k: the surviving area is a multiple of 16.  The objects therefore sit at 6400 exactly
    (20 x 20 source pixels), at the nearest area below it (6384), further away on both sides, with arms and speckle that the
    opening removes - and 6399 against 6400, which no x4 plane can have, is held at upscale = 1 on a 480 x 640 plane: an 80 x 80 square
    and the same square without one corner pixel."""
    H, W = 120, 160
    m = np.zeros((8, H, W), bool)
    m[0, 10:30, 20:40] = True                                    # 20 x 20: 6400 after the upscale
    m[1, 10:31, 20:39] = True                                    # 21 x 19 = 399 source pixels: 6384
    m[2, 50:90, 60:130] = True                                   # far above
    m[3, 5:15, 5:15] = True                                      # far below
    m[4, 10:30, 20:40] = True
    m[4, 19, 40:150] = True                                      # the 6400 square with an arm one source pixel (4 < 7) thick: removed
    m[5, 0:20, 140:160] = True                                   # 6400 in the top right corner of the frame
    m[6, 40:60, 40:59] = True                                    # 20 x 19 = 6080 ..
    m[6, 40:60, 60] = True                                       # .. and a column beside it, apart by one pixel: removed
    rs = np.random.RandomState(4)
    vv, uu = np.mgrid[0:H, 0:W]
    m[7] = (rs.rand(H, W) < 0.6) & (vv % 2 == 0) & (uu % 2 == 0)   # speckle of single pixels, no two adjacent: nothing survives
    keep, params, stats, opened = la.select_crops(planes_of(la, m))
    want = opened_all(m, 7, 4)
    check_planes(opened, stats, want, 4 * H, 4 * W, 4 * W, "gate")
    areas = [int(w.sum()) for w in want]
    assert areas[:7] == [6400, 6384, 16 * 40 * 70, 1600, 6400, 6400, 6080] and areas[7] == 0, areas
    assert keep.dtype == bool and keep.tolist() == [a >= 6400 for a in areas] == [True, False, True, False, True, True, False, False]
    rule = np.array([OC.crop_rule(*OC.rect_stats(w)[1:]) for w in want])
    assert params.dtype == np.float64 and params.shape == (8, 3)
    np.testing.assert_array_equal(params, rule)                  # (NaN rows equal in place)
    assert np.isnan(params[7]).all() and np.isfinite(params[:7]).all()
    # 6399 against 6400, at upscale 1
    big = np.zeros((2, 480, 640), bool)
    big[:, 100:180, 300:380] = True
    big[1, 100, 300] = False
    keep1, params1, stats1, opened1 = la.select_crops(planes_of(la, big), upscale=1)
    want1 = opened_all(big, 7, 1)
    assert [int(w.sum()) for w in want1] == [6400, 6399]
    check_planes(opened1, stats1, want1, 480, 640, 640, "gate s=1")
    assert keep1.tolist() == [True, False]
    np.testing.assert_array_equal(params1, [OC.crop_rule(*OC.rect_stats(w)[1:], upscale=1) for w in want1])
    assert la.select_crops(planes_of(la, big), upscale=1, min_area=6399)[0].tolist() == [True, True]


# ------------------------------------------------------------------------------------------
# 8. one call captured into a graph
# ------------------------------------------------------------------------------------------
def test_one_call_captured_into_a_graph(la):
    import ctypes as C

    import torch

    from labelany3d_amd import _lib

    H, W, B, k, s = 33, 47, 8, 3, 2
    rs = np.random.RandomState(41)
    masks = np.stack([OC.blob_plane(rs, H, W) for _ in range(B)])
    src = planes_of(la, masks, False)
    eager, eager_stats = la.open_bits(src, k=k, upscale=s, return_stats=True)
    W_out = OC.padded(s * W)
    dev = torch.device("cuda", 0)
    out = torch.zeros((B, (s * H * W_out + 31) // 32), dtype=torch.int32, device=dev)
    stats = torch.zeros((B, 5), dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.lib.la3d_open_bits_workspace_bytes(B, H, s) // 4, dtype=torch.int32, device=dev)

    def run(stream):
        rc = _lib.lib.la3d_open_bits(C.c_void_p(src.bits.data_ptr()), src.bits.stride(0), B, H, W, W, k, s, C.c_void_p(out.data_ptr()),
                                     out.stride(0), W_out, C.c_void_p(stats.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(stream.cuda_stream))
        assert rc == 0, _lib.lib.la3d_last_error()

    side = torch.cuda.Stream(device=dev)
    gr = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        run(side)                                                # (warm-up)
        side.synchronize()
        with torch.cuda.graph(gr, stream=side):
            run(torch.cuda.current_stream())
    out.fill_(SENTINEL)
    stats.fill_(-1)
    torch.cuda.synchronize()
    gr.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u32(out), u32(eager.bits))
    np.testing.assert_array_equal(np_(stats), np_(eager_stats))
    check_planes(la.MaskBits(out, s * H, W_out, s * W), stats, opened_all(masks, k, s), s * H, s * W, W_out, "replay")
