"""GPU tests of the frames form of morphology on bit planes (include/la3d.h "morphology on bit planes", la3d_open_bits_frames;
``open_bits_frames``, ``bits_rects_frames``, ``select_crops_frames``): the planes of images of different sizes opened in ONE call,
bit for bit against the NumPy restatement of the rule (tests/open_bits_cases.py), against what SciPy gave
(tests/golden/g19_opening.npz) and against the uniform ``open_bits`` on each image alone; exactly the plane's words written; the
rows the device refuses; foreign bits and a dirty workspace; the two layouts; the consumers; the crop gate; batch sizes; one
captured call."""
import ctypes as C

import numpy as np
import pytest

from . import instance_points_cases as IC
from . import open_bits_cases as OC
from . import frames_fault_rows as FR
from . import open_bits_frames_cases as FC

pytestmark = pytest.mark.gpu

SENTINEL = OC.SENTINEL
REFUSED = [-1, 0, 0, 0, 0]


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


def packed(la, masks, sizes=FC.SIZES, per_image=FC.PER_IMAGE):
    """planes in image order, per_image of each -> (PackedMasks, FrameBits); the PackedMasks is the ``frames`` of the calls"""
    pm = la.pack_mask_frames(FC.stacks(masks, sizes, per_image))
    return pm, la.pack_mask_bits_frames(pm)


def plane_of(fb, n, h, w):
    """the words of plane n of a FrameBits, an image of (h, w)"""
    o = int(np_(fb.offsets)[n])
    return u32(fb.bits)[o:o + FC.plane_words(h, w)]


def check_frames(fb, stats, want, tag):
    """fb: the opened FrameBits; want: the expected bool masks, one per row, each of its own size"""
    offs = np_(fb.offsets)
    assert len(offs) == len(want) and (offs % 4 == 0).all(), tag
    for n, m in enumerate(want):
        np.testing.assert_array_equal(plane_of(fb, n, *m.shape), FC.frame_words(m), err_msg=f"{tag}[{n}] {m.shape}")
    rects = np.array([OC.rect_stats(m) for m in want], np.int32).reshape(len(want), 5)
    if stats is not None:
        assert stats.dtype.is_floating_point is False and tuple(stats.shape) == (len(want), 5), tag
        np.testing.assert_array_equal(np_(stats), rects, err_msg=f"{tag} stats")
    np.testing.assert_array_equal(np_(fb.area), rects[:, 0], err_msg=f"{tag} area")


_OPENED = {}


def opened(k, s):
    """the NumPy-opened planes of the shared case (k, s): computed once, shared, never changed"""
    if (k, s) not in _OPENED:
        _OPENED[k, s] = (FC.planes(k, s), [OC.opening(m, k, s) for m in FC.planes(k, s)])
    return _OPENED[k, s]


def ptr(t, words=0):
    return C.c_void_p(t.data_ptr() + 4 * words)


def c_open(la, bits, bits_words, offs, table, P, H, W, ii, B, k, s, out, out_words, ooffs, stats, ws, stream=None):
    """the C entry on device tensors or ready c_void_p values"""
    import torch

    from labelany3d_amd import _lib

    p = [x if x is None or isinstance(x, C.c_void_p) else ptr(x) for x in (bits, offs, table, ii, out, ooffs, stats, ws)]
    st = torch.cuda.current_stream() if stream is None else stream
    rc = _lib.lib.la3d_open_bits_frames(p[0], bits_words, p[1], p[2], P, H, W, p[3], B, k, s, p[4], out_words, p[5], p[6], p[7],
                                        C.c_void_p(st.cuda_stream))
    assert rc == 0, _lib.lib.la3d_last_error()


def workspace(la, B, H, s, fill=None):
    import torch

    from labelany3d_amd import _lib

    n = max(int(_lib.lib.la3d_open_bits_frames_workspace_bytes(B, H, s)) // 4, 1)
    return torch.empty(n, dtype=torch.int32, device="cuda") if fill is None else torch.full((n,), fill, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------
# 1. the mixed list, bit for bit
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", FC.KS)
@pytest.mark.parametrize("s", FC.SCALES)
def test_mixed_sizes_bit_for_bit(la, k, s):
    """24 planes of 12 sizes in one call: every plane and statistics row is the restatement's, and what the uniform ``open_bits`` gives
    for that image alone"""
    import torch

    masks, want = opened(k, s)
    pm, fb = packed(la, masks)
    res, stats = la.open_bits_frames(pm, fb, k=k, upscale=s, image_index=FC.IMAGE_INDEX, return_stats=True)
    assert isinstance(res, la.FrameBits) and res.image_index is fb.image_index
    grid = la.scaled_frames(pm, s)
    assert (res.H, res.W) == (grid.H, grid.W) and np.array_equal(res.table, grid.table_host)
    assert s != 1 or ((res.H, res.W) == (pm.H, pm.W) and np.array_equal(res.table, pm.table_host))
    np.testing.assert_array_equal(np_(res.offsets), la.frame_bits_offsets(grid.table_host, FC.IMAGE_INDEX)[0])
    check_frames(res, stats, want, f"k={k} s={s}")
    for p, (h, w) in enumerate(FC.SIZES):
        rows = np.flatnonzero(FC.IMAGE_INDEX == p)
        one = la.pack_mask_bits(torch.as_tensor(np.stack([masks[n] for n in rows]).astype(np.uint8), device="cuda"), frame_pad=True)
        mb, st = la.open_bits(one, k=k, upscale=s, frame_pad=True, return_stats=True)
        assert (mb.H, mb.W, mb.frame_width) == (s * h, OC.padded(s * w), s * w)
        for j, n in enumerate(rows):
            np.testing.assert_array_equal(plane_of(res, n, s * h, s * w), u32(mb.bits)[j, :FC.plane_words(s * h, s * w)], err_msg=f"uniform {p}/{j}")
        np.testing.assert_array_equal(np_(stats)[rows], np_(st), err_msg=f"uniform stats {p}")


# ------------------------------------------------------------------------------------------
# 2. SciPy's bits
# ------------------------------------------------------------------------------------------
def test_scipy_planes_in_one_mixed_call(la, g):
    """the three frames of the fixture, four planes each, in one call per (k, s): SciPy's own outputs"""
    cases = OC.fixture_cases()
    for k in OC.KS:
        for s in OC.SCALES:
            ins, outs = [], []
            for f in range(len(OC.FRAMES)):
                a, b = OC.golden_case(g, cases.index((f, k, s)))
                ins += list(a)
                outs += list(b)
            pm, fb = packed(la, ins, OC.FRAMES, OC.PLANES)
            res, stats = la.open_bits_frames(pm, fb, k=k, upscale=s, return_stats=True)      # (the uniform-stride layout)
            check_frames(res, stats, outs, f"scipy k={k} s={s}")


# ------------------------------------------------------------------------------------------
# 3. exactly the plane's words
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s", [(7, 1), (3, 2), (7, 4)])
def test_exactly_the_words_of_each_plane_are_written(la, k, s):
    import torch

    masks, want = opened(k, s)
    pm, fb = packed(la, masks)
    B = len(masks)
    words = [FC.plane_words(*m.shape) for m in want]
    gaps = [4 * (1 + n % 3) for n in range(B)]                                   # hand-made offsets: multiples of 4, gaps between planes
    offs, at = [], 8
    for n in range(B):
        offs.append(at)
        at += (words[n] + 3) // 4 * 4 + gaps[n]
    out = torch.full((at + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    stats = torch.full((B, 5), -7, dtype=torch.int32, device="cuda")
    c_open(la, fb.bits, fb.bits.numel(), fb.offsets, pm.table, len(FC.SIZES), pm.H, pm.W, fb.image_index, B, k, s, out, out.numel(),
           torch.as_tensor(np.array(offs, np.int64), device="cuda"), stats, workspace(la, B, pm.H, s))
    expect = np.full(at + 8, SENTINEL, np.uint32)
    for n, m in enumerate(want):
        expect[offs[n]:offs[n] + words[n]] = FC.frame_words(m)                   # (padding columns zero)
    np.testing.assert_array_equal(u32(out), expect)
    np.testing.assert_array_equal(np_(stats), [OC.rect_stats(m) for m in want])


# ------------------------------------------------------------------------------------------
# 4. refused rows
# ------------------------------------------------------------------------------------------
def test_refused_rows_write_nothing_and_say_so(la):
    """One bad value per refused row - the shared case table (tests/frames_fault_rows.py) and the faults of the output, which are this
    entry's own; every address a defect would form from it lies inside this test's own allocations (the table, the input and the
    output have pad in front and behind), so a defect shows as a changed word, never as a fault."""
    import torch

    k, s = 3, 2
    rs = np.random.RandomState(4)
    OUT, PAD = 512, FR.PAD                                                       # output slots of 512 words hold every scaled plane
    c = FR.case(end_check=True, extra=[(1, "output offset 6"), (2, "output offset -4"), (0, "output plane ends one word past out_words")])
    rows, B, P, H, W, good = c.rows, c.B, c.P, c.H, c.W, FR.GOOD
    bits_words, out_words = c.words, B * OUT + 1
    ioffs, ooffs = c.offsets, np.arange(B, dtype=np.int64) * OUT
    for n, (img, bad) in enumerate(rows):
        if bad == "output offset 6":
            ooffs[n] += 6
        elif bad == "output offset -4":
            ooffs[n] = -4
        elif bad == "output plane ends one word past out_words":
            ooffs[n] = out_words - FC.plane_words(s * good[img][0], s * good[img][1]) + 1
            assert ooffs[n] % 4 == 0 and ooffs[n] >= 0
    masks = {n: OC.blob_plane(rs, *good[rows[n][0]]) for n in c.good}
    inbuf = FR.input_words(c, rs, lambda n, h, w: FC.frame_words(masks[n]))      # garbage wherever no plane lies
    d = FR.on_device(c, inbuf)
    inp, table, ii = d.bits_all, d.table_all, d.image_index
    out = torch.full((PAD + out_words + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    stats = torch.full((B, 5), -7, dtype=torch.int32, device="cuda")
    c_open(la, ptr(inp, PAD), bits_words, torch.as_tensor(ioffs, device="cuda"), C.c_void_p(table.data_ptr() + 24), P, H, W, ii, B, k, s,
           ptr(out, PAD), out_words, torch.as_tensor(ooffs, device="cuda"), stats, workspace(la, B, H, s))
    expect = np.full(PAD + out_words + PAD, SENTINEL, np.uint32)
    want_stats = []
    for n, (img, bad) in enumerate(rows):
        if bad is None:
            m = OC.opening(masks[n], k, s)
            wds = FC.frame_words(m)
            expect[PAD + ooffs[n]:PAD + ooffs[n] + len(wds)] = wds
            want_stats.append(OC.rect_stats(m))
        else:
            want_stats.append(REFUSED)
    got = np_(stats).tolist()
    for n, (img, bad) in enumerate(rows):
        assert got[n] == want_stats[n], (n, bad, got[n])
    changed = np.flatnonzero(u32(out) != expect)
    assert not len(changed), (changed[:8] - PAD, [(n, bad) for n, (_, bad) in enumerate(rows) if bad])
    np.testing.assert_array_equal(u32(inp), inbuf)
    assert sum(bad is None for _, bad in rows) == 6 and any(r[0] > 0 for r in want_stats)
    assert {bad for _, bad in rows} >= set(FR.INDEX_FAULTS + FR.OFFSET_FAULTS + [FR.END_FAULT] + [f for f, _ in FR.FRAME_FAULTS])
    # the statistics-only call makes the same decisions, but for the rows whose only fault lies in the output
    stats1 = torch.full((B, 5), -7, dtype=torch.int32, device="cuda")
    c_open(la, ptr(inp, PAD), bits_words, torch.as_tensor(ioffs, device="cuda"), C.c_void_p(table.data_ptr() + 24), P, H, W, ii, B, 1, 1,
           None, 0, None, stats1, workspace(la, B, H, 1))
    got1 = np_(stats1).tolist()
    for n, (img, bad) in enumerate(rows):
        if bad is None:
            assert got1[n] == OC.rect_stats(masks[n]), n
        elif "output" not in bad:
            assert got1[n] == REFUSED, (n, bad)


def test_no_image_refuses_every_row(la):
    """P == 0 with B > 0: no frame row is ever addressed; every statistics row says refused and no plane word is written"""
    import torch

    B = 3
    bits = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.full((256,), SENTINEL, dtype=torch.int32, device="cuda")
    offs = torch.arange(B, dtype=torch.int64, device="cuda") * 16
    stats = torch.full((B, 5), -7, dtype=torch.int32, device="cuda")
    c_open(la, bits, 64, offs, None, 0, 8, 32, torch.zeros(B, dtype=torch.int32, device="cuda"), B, 3, 1, out, 256, offs, stats,
           workspace(la, B, 8, 1))
    assert np_(stats).tolist() == [REFUSED] * B and (u32(out) == SENTINEL).all()


# ------------------------------------------------------------------------------------------
# 5. foreign bits
# ------------------------------------------------------------------------------------------
def test_foreign_bits_in_padding_and_between_planes_are_ignored(la):
    import torch

    k, s = 7, 2
    masks, want = opened(k, s)
    pm, fb = packed(la, masks)
    offs = np_(fb.offsets)
    dirty = np.random.RandomState(9).randint(0, 2 ** 32, fb.bits.numel(), dtype=np.uint64).astype(np.uint32)    # garbage between the planes
    set_pad = 0
    for n, m in enumerate(masks):
        h, w = m.shape
        pad = np.ones((h, OC.padded(w)), bool)
        pad[:, :w] = m                                                           # every padding column set
        wds = OC.words(pad, OC.padded(w))
        set_pad += int(np.bitwise_xor(wds, FC.frame_words(m)).any())
        dirty[offs[n]:offs[n] + len(wds)] = wds
    assert set_pad == 12 and (dirty != u32(fb.bits)).any()
    fb2 = fb._replace(bits=torch.as_tensor(dirty.view(np.int32), device="cuda"))
    for idx in (FC.IMAGE_INDEX, None):
        res, stats = la.open_bits_frames(pm, fb2, k=k, upscale=s, image_index=idx, return_stats=True)
        check_frames(res, stats, want, f"dirty layout={'compact' if idx is not None else 'stride'}")
    np.testing.assert_array_equal(np_(la.bits_rects_frames(pm, fb2)), [OC.rect_stats(m) for m in masks])


# ------------------------------------------------------------------------------------------
# 6. the workspace
# ------------------------------------------------------------------------------------------
def test_statistics_do_not_depend_on_what_the_workspace_held(la):
    """a 1-band image and a 5-band image (16 and 280 output rows in bands of 64): the short instance must read its own record only"""
    import torch

    k, s = 7, 2
    sizes = [(8, 33), (140, 96)]
    rs = np.random.RandomState(6)
    masks = [OC.blob_plane(rs, *sizes[p]) for p in (0, 0, 1, 1)]
    masks[0][:] = True                                                           # a plane that survives: its record matters
    pm, fb = packed(la, masks, sizes, 2)
    B = 4
    got = []
    for fill in (0, 0x7fffffff, -1, 0x7fffff00):
        ws = workspace(la, B, pm.H, s, fill)
        if fill == 0x7fffff00:
            ws.view(-1)[::8] = 0x7fffffff                                        # areas that would overflow any sum, rectangles that win any min / max
            ws.view(-1)[1::8] = -5
        stats = torch.full((B, 5), -7, dtype=torch.int32, device="cuda")
        c_open(la, fb.bits, fb.bits.numel(), fb.offsets, pm.table, 2, pm.H, pm.W, fb.image_index, B, k, s, None, 0, None, stats, ws)
        got.append(np_(stats).tolist())
    want = [OC.rect_stats(OC.opening(m, k, s)) for m in masks]
    assert want[0][0] == 16 * 66 and want[2][0] > 0
    for fill, st in zip(("0", "7fffffff", "-1", "mixed"), got):
        assert st == want, fill


# ------------------------------------------------------------------------------------------
# 7. layouts
# ------------------------------------------------------------------------------------------
def test_layouts_and_partial_calls_agree(la):
    import torch

    k, s = 7, 4
    masks, want = opened(k, s)
    pm, fb = packed(la, masks)
    compact, st_c = la.open_bits_frames(pm, fb, k=k, upscale=s, image_index=FC.IMAGE_INDEX, return_stats=True)
    strided, st_s = la.open_bits_frames(pm, fb, k=k, upscale=s, return_stats=True)
    check_frames(compact, st_c, want, "compact")
    check_frames(strided, st_s, want, "stride")
    grid = la.scaled_frames(pm, s)
    stride = (grid.H * grid.W // 32 + 3) // 4 * 4
    assert np_(strided.offsets).tolist() == [n * stride for n in range(len(masks))]
    assert compact.bits.numel() < strided.bits.numel()
    np.testing.assert_array_equal(np_(compact.offsets), la.frame_bits_offsets(grid.table_host, FC.IMAGE_INDEX)[0])
    # a torch host index, and out=
    out = torch.full((compact.bits.numel() + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    plain = la.open_bits_frames(pm, fb, k=k, upscale=s, image_index=torch.as_tensor(FC.IMAGE_INDEX), out=out)      # return_stats=False
    assert isinstance(plain, la.FrameBits) and plain.bits is out
    check_frames(plain, None, want, "no stats")
    with pytest.raises(ValueError, match="overlaps"):
        la.open_bits_frames(pm, fb, k=k, upscale=s, out=fb.bits)
    with pytest.raises(ValueError, match="out must be"):
        la.open_bits_frames(pm, fb, k=k, upscale=s, image_index=FC.IMAGE_INDEX, out=out[:64])
    # out_bits = NULL through the C entry: the same statistics, nothing else written
    stats = torch.full((len(masks), 5), -7, dtype=torch.int32, device="cuda")
    c_open(la, fb.bits, fb.bits.numel(), fb.offsets, pm.table, len(FC.SIZES), pm.H, pm.W, fb.image_index, len(masks), k, s, None, 0, None,
           stats, workspace(la, len(masks), pm.H, s))
    np.testing.assert_array_equal(np_(stats), np_(st_c))
    # planes without statistics through the C entry
    out2 = torch.full_like(out, SENTINEL)
    c_open(la, fb.bits, fb.bits.numel(), fb.offsets, pm.table, len(FC.SIZES), pm.H, pm.W, fb.image_index, len(masks), k, s, out2, out2.numel(),
           compact.offsets, None, None)
    np.testing.assert_array_equal(u32(out2), u32(out))
    np.testing.assert_array_equal(np_(la.bits_rects_frames(grid, compact)), np_(st_c))        # a FrameGrid as ``frames``


# ------------------------------------------------------------------------------------------
# 8. consumers
# ------------------------------------------------------------------------------------------
def test_consumers_take_the_opened_planes(la):
    k = 7
    masks, want = opened(k, 1)
    pm, fb = packed(la, masks)
    P = len(FC.SIZES)
    rs = np.random.RandomState(2)
    pf = la.pack_frames([rs.uniform(0.5, 10.0, hw).astype(np.float32) for hw in FC.SIZES])
    K = np.stack([IC.cameras(1, h, w)[0] for h, w in FC.SIZES])
    res = la.open_bits_frames(pm, fb, k=k, image_index=FC.IMAGE_INDEX)
    got = la.fit_instances_frames_bits(pf, res, K)                              # x1: the caller's own frames
    ref = la.fit_instances_frames_bits(pf, packed(la, want)[1], K)
    np.testing.assert_array_equal(np_(got["status"]), np_(ref["status"]))
    np.testing.assert_array_equal(np_(got["boxes"]), np_(ref["boxes"]))          # (NaN == NaN in the same place)
    assert np.isfinite(np_(ref["boxes"])).any() and P == 12
    # x4: the run lengths of the scaled grid decode to the opened masks
    masks4, want4 = opened(k, 4)
    pm4, fb4 = packed(la, masks4)
    res4 = la.open_bits_frames(pm4, fb4, k=k, upscale=4)
    grid = la.scaled_frames(pm4, 4)
    (counts, offsets), sizes = la.rle_encode_bits_frames(grid, res4)
    objs = la.rle_objects((counts, offsets), sizes=sizes)
    assert len(objs) == len(want4)
    for n, (o, m) in enumerate(zip(objs, want4)):
        assert o["size"] == list(m.shape), n
        runs = np.asarray(o["counts"], np.int64)
        assert runs.sum() == m.size
        vals = np.zeros(len(runs), bool)
        vals[1::2] = True
        np.testing.assert_array_equal(np.repeat(vals, runs).reshape(m.shape[::-1]).T, m, err_msg=f"runs {n}")   # column-major


# ------------------------------------------------------------------------------------------
# 9. the crop gate
# ------------------------------------------------------------------------------------------
def test_select_crops_frames_is_select_crops_per_image(la):
    import torch

    masks, _ = opened(7, 4)
    pm, fb = packed(la, masks)
    bad = 5                                                                      # one row the device refuses: an offset that is no multiple of 4
    offs = np_(fb.offsets).copy()
    offs[bad] += 2
    fb = fb._replace(offsets=torch.as_tensor(offs, device="cuda"))
    S = 64
    keep, params, stats, res = la.select_crops_frames(pm, fb, crop_size=S, image_index=FC.IMAGE_INDEX)
    assert keep.dtype == bool and keep.shape == (24,) and params.dtype == np.float64 and params.shape == (24, 3)
    st = np_(stats)
    for p, (h, w) in enumerate(FC.SIZES):
        rows = np.flatnonzero(FC.IMAGE_INDEX == p)
        one = la.pack_mask_bits(torch.as_tensor(np.stack([masks[n] for n in rows]).astype(np.uint8), device="cuda"), frame_pad=True)
        k1, p1, s1, _ = la.select_crops(one, crop_size=S)
        for j, n in enumerate(rows):
            if n == bad:
                assert st[n].tolist() == REFUSED and not keep[n] and np.isnan(params[n]).all()
                continue
            assert keep[n] == k1[j] and st[n].tolist() == np_(s1)[j].tolist(), n
            np.testing.assert_array_equal(params[n], p1[j], err_msg=f"row {n}")  # exact; NaN rows equal in place
    empty = st[:, 0] == 0
    assert keep.any() and (~keep).any() and empty.any() and np.isnan(params[empty]).all() and not keep[empty].any()
    assert (keep == (st[:, 0] >= 6400)).all() and np.isfinite(params[st[:, 0] > 0]).all()
    assert la.select_crops_frames(pm, fb, crop_size=S, min_area=0)[0].tolist() == (st[:, 0] >= 0).tolist()
    # the parameters speak of the original frames: pack_crop_bits_frames takes them, and restores what pack_crop_bits restores
    pf = la.pack_frames([np.ones(hw, np.float32) for hw in FC.SIZES])
    sel = np.flatnonzero(keep)
    crops = torch.ones((len(sel), S, S), dtype=torch.uint8, device="cuda")
    back = la.pack_crop_bits_frames(pf, crops, params[sel], FC.IMAGE_INDEX[sel])
    for j, n in enumerate(sel):
        h, w = FC.SIZES[FC.IMAGE_INDEX[n]]
        one = la.pack_crop_bits(crops[j:j + 1], params[n:n + 1], (w, h))
        np.testing.assert_array_equal(plane_of(back, j, h, w), u32(one.bits)[0, :FC.plane_words(h, w)], err_msg=f"crop {n}")
        assert int(np_(back.area)[j]) > 0


# ------------------------------------------------------------------------------------------
# 10. batch sizes
# ------------------------------------------------------------------------------------------
def test_empty_batches(la):
    import torch

    from labelany3d_amd.frames import _table_fields, frame_table

    def empty(sizes):
        grid = la.FrameGrid(*_table_fields(frame_table(sizes), sizes, torch.device("cuda", 0)))
        z = torch.zeros(0, dtype=torch.int32, device="cuda")
        return grid, la.FrameBits(torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"), z, z,
                                  grid.table_host, grid.H, grid.W)

    for frames, bits in (empty(list(FC.SIZES)), empty([])):                      # B = 0; P = 0 with B = 0
        for s in (1, 4):
            res, stats = la.open_bits_frames(frames, bits, k=7, upscale=s, return_stats=True)
            assert tuple(stats.shape) == (0, 5) and res.offsets.numel() == 0 and res.area.numel() == 0
            res = la.open_bits_frames(frames, bits, k=7, upscale=s, image_index=np.zeros(0, np.int32))
            assert res.offsets.numel() == 0 and (res.H, res.W) == (s * frames.H, la.scaled_frames(frames, s).W)
        assert tuple(la.bits_rects_frames(frames, bits).shape) == (0, 5)
        keep, params, stats, _ = la.select_crops_frames(frames, bits)
        assert keep.shape == (0,) and params.shape == (0, 3) and tuple(stats.shape) == (0, 5)
    torch.cuda.synchronize()


def test_three_hundred_rows_drawn_from_the_list(la):
    k, s = 5, 2
    rs = np.random.RandomState(300)
    per = 25                                                                     # 12 sizes x 25 = 300 rows
    base = {p: [OC.blob_plane(rs, *FC.SIZES[p]) for _ in range(3)] for p in range(len(FC.SIZES))}
    masks = []
    for p, (h, w) in enumerate(FC.SIZES):
        for j in range(per):
            m = base[p][j % 3].copy()
            m[j % h, :] ^= True                                                  # few planes alike
            masks.append(m)
    assert len(masks) == 300
    pm, fb = packed(la, masks, FC.SIZES, per)
    cache = {}
    want = []
    for m in masks:
        key = m.tobytes() + bytes(m.shape)
        if key not in cache:
            cache[key] = OC.opening(m, k, s)
        want.append(cache[key])
    res, stats = la.open_bits_frames(pm, fb, k=k, upscale=s, image_index=np.repeat(np.arange(len(FC.SIZES)), per), return_stats=True)
    check_frames(res, stats, want, "B=300")


def test_all_rows_of_one_image_equal_the_uniform_call(la):
    import torch

    h, w, B, k, s = 40, 50, 9, 5, 2
    rs = np.random.RandomState(11)
    masks = [OC.blob_plane(rs, h, w) for _ in range(B)]
    pm, fb = packed(la, masks, [(h, w)], B)
    res, stats = la.open_bits_frames(pm, fb, k=k, upscale=s, return_stats=True)
    mb, st = la.open_bits(la.pack_mask_bits(torch.as_tensor(np.stack(masks).astype(np.uint8), device="cuda"), frame_pad=True), k=k, upscale=s,
                          return_stats=True)
    nw = FC.plane_words(s * h, s * w)
    for n in range(B):
        np.testing.assert_array_equal(plane_of(res, n, s * h, s * w), u32(mb.bits)[n, :nw], err_msg=f"plane {n}")
    np.testing.assert_array_equal(np_(stats), np_(st))
    check_frames(res, stats, [OC.opening(m, k, s) for m in masks], "one image")


# ------------------------------------------------------------------------------------------
# 11. one call captured into a graph
# ------------------------------------------------------------------------------------------
def test_one_call_captured_into_a_graph(la):
    """a single linear chain - the band kernel, then the statistics kernel -, replayed after the input planes changed"""
    import torch

    k, s = 7, 2
    first, _ = opened(k, s)
    second, want2 = opened(15, 2)                                                # other planes of the same sizes
    pm, fb = packed(la, first)
    fb2 = packed(la, second)[1]
    assert np.array_equal(np_(fb.offsets), np_(fb2.offsets))
    B, P = len(first), len(FC.SIZES)
    want2 = [OC.opening(m, k, s) for m in second]
    dev = torch.device("cuda", 0)
    grid = la.scaled_frames(pm, s)
    offs_h, total = la.frame_bits_offsets(grid.table_host, FC.IMAGE_INDEX)
    ooffs = torch.as_tensor(offs_h, device=dev)
    out = torch.zeros(total, dtype=torch.int32, device=dev)
    stats = torch.zeros((B, 5), dtype=torch.int32, device=dev)
    ws = workspace(la, B, pm.H, s)
    src = fb.bits.clone()

    def run(stream):
        c_open(la, src, src.numel(), fb.offsets, pm.table, P, pm.H, pm.W, fb.image_index, B, k, s, out, total, ooffs, stats, ws, stream)

    side = torch.cuda.Stream(device=dev)
    gr = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        run(side)                                                                # (warm-up)
        side.synchronize()
        with torch.cuda.graph(gr, stream=side):
            run(torch.cuda.current_stream())
    src.copy_(fb2.bits)
    out.fill_(SENTINEL)
    stats.fill_(-1)
    torch.cuda.synchronize()
    gr.replay()
    torch.cuda.synchronize()
    res = la.FrameBits(out, ooffs, fb.image_index, stats[:, 0].contiguous(), grid.table_host, grid.H, grid.W)
    check_frames(res, stats, want2, "replay")
