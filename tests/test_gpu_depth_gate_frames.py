"""GPU tests of the frames form of the depth gate on bit planes (include/la3d.h "depth gate on bit planes",
la3d_depth_gate_bits_frames; ``gate_depth_bits_frames``, ``depth_gate_stats_frames``): the planes of images of different sizes gated
in ONE call over float32, float16 and uint16 depth - planes and counts exact and levels equal against ``depth_gate_cases.gate`` applied
row by row (tests/depth_gate_frames_cases.py), word for word against the float32 call on unpacked planes and against the uniform
``gate_depth_bits``; exactly the plane's words written; the rows the device refuses; in place, statistics only, two runs; one captured
call; the fit downstream; the case the feature exists for."""
import ctypes as C

import numpy as np
import pytest

from . import depth16_cases as D16
from . import depth_gate_cases as DG
from . import depth_gate_frames_cases as XG
from . import frames_fault_rows as FR
from . import instance_points_cases as IC
from . import open_bits_frames_cases as OF

pytestmark = pytest.mark.gpu

SENTINEL = DG.SENTINEL
REFUSED = XG.REFUSED_COUNTS


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def np_(t):
    return t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()


def u32(t):
    return np_(t).view(np.uint32)


def dev(a):
    import torch

    return torch.as_tensor(np.array(a), device="cuda")              # (a copy: the shared cases are read-only)


_PACKED = {}


def packed_bits(la, key, row_masks, ii, P):
    """rows in image order -> (PackedMasks, FrameBits), packed once per key and shared: no test writes into either"""
    key = ("bits", key)
    if key not in _PACKED:
        pm = la.pack_mask_frames(XG.stacks(row_masks, ii, P))
        _PACKED[key] = pm, la.pack_mask_bits_frames(pm)
    return _PACKED[key]


def packed_depth(la, key, maps, variant=None):
    """one map per image -> PackedFrames, or - maps already 16-bit, ``variant`` of depth16_cases - PackedFrames16; packed once per key"""
    key = ("depth", key)
    if key not in _PACKED:
        maps = [np.array(m) for m in maps]
        _PACKED[key] = la.pack_frames(maps) if variant is None else la.pack_frames(maps, dtype=variant[0], scale=variant[1], zero_is_hole=variant[2])
    return _PACKED[key]


def unpacked(la, pf16):
    """the float32 PackedFrames a caller without the 16-bit form makes: ``unpack_depth16`` of the whole buffer, the same table"""
    flat = la.unpack_depth16(la.Depth16(pf16.data.view(1, -1), pf16.scale, pf16.zero_is_hole)).view(-1)
    return la.PackedFrames(flat, pf16.table, pf16.table_host, pf16.H, pf16.W, pf16.sizes)


def plane_of(bits, offsets, n, h, w):
    o = int(np_(offsets)[n])
    return u32(bits)[o:o + XG.plane_words(h, w)]


def check(res, stats, want, tag, fb=None):
    """res: the FrameBits of a call; stats: its DepthGateStats; want: (keeps, counts, levels) of the oracle"""
    keeps, counts, levels = want
    assert len(np_(res.offsets)) == len(keeps), tag
    for n, m in enumerate(keeps):
        np.testing.assert_array_equal(plane_of(res.bits, res.offsets, n, *m.shape), XG.frame_words(m), err_msg=f"{tag}[{n}] {m.shape}")   # (pad columns zero)
    if stats is not None:
        got_counts, got_levels = np_(stats.counts), np_(stats.levels)
        assert got_counts.dtype == np.int32 and got_levels.dtype == np.float32 and got_counts.shape == got_levels.shape == (len(keeps), 3), tag
        np.testing.assert_array_equal(got_counts, counts, err_msg=f"{tag} counts")
        np.testing.assert_array_equal(got_levels, levels, err_msg=f"{tag} levels")          # (NaN == NaN in the same place)
    np.testing.assert_array_equal(np_(res.area), np.maximum(counts[:, 2], 0), err_msg=f"{tag} area")
    if fb is not None:
        assert res.offsets is fb.offsets and res.image_index is fb.image_index and res.table is fb.table and (res.H, res.W) == (fb.H, fb.W), tag


def mixed(la):
    return packed_depth(la, "mixed f32", XG.depth_maps()), packed_bits(la, "mixed", XG.masks(), XG.IMAGE_INDEX, len(XG.SIZES))[1]


def ptr(t, elems=0, size=4):
    return C.c_void_p(t.data_ptr() + size * elems)


def c_gate(depth, depth_elems, table, P, H, W, ii, B, bits, bits_words, offs, out, out_words, ooffs, counts, levels, d16=None, stream=None,
           k=4.5, min_band=0.0, near=-DG.INF, far=DG.INF):
    """the C entry on device tensors or ready c_void_p values; ``d16``: (dtype code, scale, flags) of a 16-bit depth buffer"""
    import torch

    from labelany3d_amd import _lib

    p = [None if x is None else (x.value if isinstance(x, C.c_void_p) else x.data_ptr()) for x in (depth, table, ii, bits, offs, out, ooffs, counts, levels)]
    st = torch.cuda.current_stream() if stream is None else stream
    blk = None
    if d16 is not None:
        blk = _lib.Depth16Block(struct_size=C.sizeof(_lib.Depth16Block), dtype=d16[0], planes=p[0], plane_stride=0, scale=d16[1], flags=d16[2])
    a = _lib.DepthGateFramesArgs(struct_size=C.sizeof(_lib.DepthGateFramesArgs), B=B, P=P, H=H, W=W, k=k, min_band=min_band, near=near, far=far,
                                 depth=None if blk is not None else p[0], depth16=None if blk is None else C.pointer(blk), depth_elems=depth_elems,
                                 frames=p[1], image_index=p[2], bits=p[3], bits_words=bits_words, bits_offsets=p[4],
                                 out_bits=p[5], out_words=out_words, out_offsets=p[6], counts=p[7], levels=p[8], stream=st.cuda_stream)
    rc = _lib.lib.la3d_depth_gate_bits_frames(C.byref(a))
    assert rc == 0, _lib.lib.la3d_last_error()


# ------------------------------------------------------------------------------------------
# 1. the mixed list, exact, under every scalar set
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", range(len(DG.PARAMS)))
def test_mixed_sizes_exact(la, pi):
    """24 planes of 12 sizes over 12 depth planes in one call: every plane, count and level is the oracle's"""
    pf, fb = mixed(la)
    res, stats = la.gate_depth_bits_frames(pf, fb, return_stats=True, **DG.PARAMS[pi])
    assert isinstance(res, la.FrameBits) and isinstance(stats, la.DepthGateStats)
    check(res, stats, XG.expected(pi), f"params {DG.PARAMS[pi]}", fb)


# ------------------------------------------------------------------------------------------
# 2. 16-bit depth where it lies
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", D16.VARIANTS, ids=D16.VARIANT_IDS)
def test_depth16_equals_the_oracle_and_the_float32_call_on_unpacked_planes(la, variant):
    _, fb = mixed(la)
    pf16 = packed_depth(la, f"mixed {variant}", XG.stored(variant), variant)
    assert isinstance(pf16, la.PackedFrames16) and pf16.data.element_size() == 2
    pf32 = unpacked(la, pf16)
    for pi in range(len(DG.PARAMS)):
        res, stats = la.gate_depth_bits_frames(pf16, fb, return_stats=True, **DG.PARAMS[pi])
        check(res, stats, XG.expected(pi, variant), f"{variant} params {DG.PARAMS[pi]}", fb)
        ref, ref_stats = la.gate_depth_bits_frames(pf32, fb, return_stats=True, **DG.PARAMS[pi])
        for n, m in enumerate(XG.masks()):                                                # word for word, plane by plane
            np.testing.assert_array_equal(plane_of(res.bits, res.offsets, n, *m.shape), plane_of(ref.bits, ref.offsets, n, *m.shape))
        np.testing.assert_array_equal(np_(stats.counts), np_(ref_stats.counts))
        np.testing.assert_array_equal(np_(stats.levels).view(np.uint32), np_(ref_stats.levels).view(np.uint32))
    only = la.depth_gate_stats_frames(pf16, fb)
    np.testing.assert_array_equal(np_(only.counts), XG.expected(0, variant)[1])


# ------------------------------------------------------------------------------------------
# 3. both selection paths
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", [None, XG.BIG_BOUNDS], ids=["frame-is-the-bounds", "frame-below-the-bounds"])
def test_both_selection_paths(la, bounds):
    """the 96 x 96 rows (counts on both sides of the 6144 keys the selection holds in LDS) among three small images"""
    sizes, depths, row_masks, ii = XG.big_list()
    pf = packed_depth(la, "big f32", depths)
    fb = packed_bits(la, "big", row_masks, ii, len(sizes))[1]
    assert (pf.H, pf.W) == (96, 96)
    if bounds is not None:                                                                # the same table under larger bounds
        pf, fb = pf._replace(H=bounds[0], W=bounds[1]), fb._replace(H=bounds[0], W=bounds[1])
    for pi in (0, 2, 5, 8):
        res, stats = la.gate_depth_bits_frames(pf, fb, return_stats=True, **DG.PARAMS[pi])
        check(res, stats, XG.big_expected(pi), f"big {bounds} params {DG.PARAMS[pi]}", fb)


# ------------------------------------------------------------------------------------------
# 4. a uniform-size FrameBits equals gate_depth_bits
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [DG.FRAMES[1][:2], DG.FRAMES[2][:2], DG.BIG])
def test_uniform_sizes_equal_gate_depth_bits(la, H, W):
    names, depths, masks = DG.big_planes() if (H, W) == DG.BIG else DG.planes(H, W)
    B, Ws = len(masks), DG.stored_width(W, True)
    pf = packed_depth(la, f"uniform {H}x{W}", list(depths))
    fb = packed_bits(la, f"uniform {H}x{W}", list(masks), np.arange(B), B)[1]
    one = la.MaskBits(dev(DG.pack(masks, Ws).view(np.int32)), H, Ws, W)
    d = dev(DG.pad_depth(depths, Ws))
    nw = XG.plane_words(H, W)
    for pi in (0, 2, 6, 9):
        res, stats = la.gate_depth_bits_frames(pf, fb, return_stats=True, **DG.PARAMS[pi])
        mb, st = la.gate_depth_bits(d, one, return_stats=True, **DG.PARAMS[pi])
        for n in range(B):
            np.testing.assert_array_equal(plane_of(res.bits, res.offsets, n, H, W), u32(mb.bits)[n, :nw], err_msg=f"plane {n} ({names[n]}) params {pi}")
        np.testing.assert_array_equal(np_(stats.counts), np_(st.counts))
        np.testing.assert_array_equal(np_(stats.levels).view(np.uint32), np_(st.levels).view(np.uint32))
        assert (np_(st.counts)[:, 1] > 0).any()


# ------------------------------------------------------------------------------------------
# 5. dirty inputs, exact writes
# ------------------------------------------------------------------------------------------
def test_garbage_in_padding_and_between_planes_and_sentinels_around_every_output(la):
    import torch

    pf, fb = mixed(la)
    masks = XG.masks()
    B = len(masks)
    offs = np_(fb.offsets)
    dirty = np.random.RandomState(9).randint(0, 2 ** 32, fb.bits.numel(), dtype=np.uint64).astype(np.uint32)    # garbage between the planes
    set_pad = 0
    for n, m in enumerate(masks):
        h, w = m.shape
        pad = np.ones((h, OF.OC.padded(w)), bool)
        pad[:, :w] = m                                                           # every padding column set
        wds = OF.OC.words(pad, OF.OC.padded(w))
        set_pad += int(np.bitwise_xor(wds, XG.frame_words(m)).any())
        dirty[offs[n]:offs[n] + len(wds)] = wds
    assert set_pad >= 12 and (dirty != u32(fb.bits)).any()
    src = torch.as_tensor(dirty.view(np.int32), device="cuda")
    words = [XG.plane_words(*m.shape) for m in masks]
    ooffs, at = [], 8
    for n in range(B):                                                           # hand-made offsets: multiples of 4, gaps between planes
        ooffs.append(at)
        at += (words[n] + 3) // 4 * 4 + 4 * (1 + n % 3)
    ooffs_d = torch.as_tensor(np.array(ooffs, np.int64), device="cuda")
    for pi in (0, 3, 7):
        keeps, want_counts, want_levels = XG.expected(pi)
        out = torch.full((at + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        counts = torch.full((B, 3), -7, dtype=torch.int32, device="cuda")
        levels = torch.full((B, 3), -7.0, dtype=torch.float32, device="cuda")
        c_gate(pf.depth, pf.depth.numel(), pf.table, len(XG.SIZES), pf.H, pf.W, fb.image_index, B, src, src.numel(), fb.offsets, out, out.numel(),
               ooffs_d, counts, levels, **DG.PARAMS[pi])
        expect = np.full(at + 8, SENTINEL, np.uint32)
        for n, m in enumerate(keeps):
            expect[ooffs[n]:ooffs[n] + words[n]] = XG.frame_words(m)             # (padding columns zero)
        np.testing.assert_array_equal(u32(out), expect, err_msg=f"params {pi}")
        np.testing.assert_array_equal(np_(counts), want_counts)
        np.testing.assert_array_equal(np_(levels), want_levels)
    np.testing.assert_array_equal(u32(src), dirty)


# ------------------------------------------------------------------------------------------
# 6. refused rows
# ------------------------------------------------------------------------------------------
def fault_depth(rs):
    """the depth buffer of the fault table's good images with pad in front and behind -> (host buffer, offsets, elements, maps)"""
    sizes = [h * FR.padded(w) for h, w in FR.GOOD]
    offsets = (0, sizes[0], sizes[0] + sizes[1])
    elems = sum(sizes)
    buf = rs.uniform(0.5, 9.0, FR.PAD + elems + FR.PAD).astype(np.float32)        # garbage wherever no plane lies
    maps = []
    for (h, w), o in zip(FR.GOOD, offsets):
        d = DG.smooth(rs, h, w)
        d.reshape(-1)[rs.permutation(h * w)[:7]] = np.array([np.nan, np.inf, DG.FILL, 7.5, 7.5, -1.0, 0.0], np.float32)
        full = np.full((h, FR.padded(w)), DG.FILL, np.float32)                    # the fill value in every padding column
        full[:, :w] = d
        buf[FR.PAD + o:FR.PAD + o + full.size] = full.reshape(-1)
        maps.append(d)
    return buf, offsets, elems, maps


def test_refused_rows_write_nothing_and_say_so(la):
    """One bad value per refused row - the shared case table (tests/frames_fault_rows.py), the faults of the output and of the depth
    buffer's length, which are this entry's own; every address a defect would form from a bad value lies inside this test's own
    allocations (table, planes, output and depth have pad in front and behind), so a defect shows as a changed word, never as a fault."""
    import torch

    rs = np.random.RandomState(4)
    SLOT, PAD = FR.SLOT, FR.PAD
    dbuf, doffs, delems, dmaps = fault_depth(rs)
    c = FR.case(end_check=True, extra=[(1, "output offset 6"), (2, "output offset -4"), (0, "output plane ends one word past out_words")],
                depth_offsets=doffs)
    rows, B, P, H, W, good = c.rows, c.B, c.P, c.H, c.W, FR.GOOD
    out_words = B * SLOT + 1
    ooffs = np.arange(B, dtype=np.int64) * SLOT
    for n, (img, bad) in enumerate(rows):
        if bad == "output offset 6":
            ooffs[n] += 6
        elif bad == "output offset -4":
            ooffs[n] = -4
        elif bad == "output plane ends one word past out_words":
            ooffs[n] = out_words - XG.plane_words(*good[img]) + 1
            assert ooffs[n] % 4 == 0 and ooffs[n] >= 0
    row_mask = {n: rs.rand(*good[rows[n][0]]) < 0.6 for n in c.good}
    inbuf = FR.input_words(c, rs, lambda n, h, w: XG.frame_words(row_mask[n]))    # garbage wherever no plane lies
    d = FR.on_device(c, inbuf)
    depth_all = torch.as_tensor(dbuf, device="cuda")
    ooffs_d = torch.as_tensor(ooffs, device="cuda")
    frames = C.c_void_p(d.table_all.data_ptr() + 24)
    kw = dict(k=3.0, min_band=0.02)

    def run(sel, out, counts, levels, elems=delems, with_out=True):
        idx = torch.as_tensor(np.asarray(sel, np.int64), device="cuda")
        c_gate(ptr(depth_all, PAD), elems, frames, P, H, W, d.image_index[idx].contiguous(), len(sel), ptr(d.bits_all, PAD), c.words,
               d.offsets[idx].contiguous(), ptr(out, PAD) if with_out else None, out_words if with_out else 0,
               ooffs_d[idx].contiguous() if with_out else None, counts, levels, **kw)

    def fresh(n):
        return (torch.full((PAD + out_words + PAD,), SENTINEL, dtype=torch.int32, device="cuda"),
                torch.full((n, 3), -7, dtype=torch.int32, device="cuda"), torch.full((n, 3), -7.0, dtype=torch.float32, device="cuda"))

    out, counts, levels = fresh(B)
    run(range(B), out, counts, levels)
    expect = np.full(PAD + out_words + PAD, SENTINEL, np.uint32)
    want_counts, want_levels = np.zeros((B, 3), np.int32), np.full((B, 3), np.nan, np.float32)
    for n, (img, bad) in enumerate(rows):
        if bad is None:
            keep, want_counts[n], want_levels[n] = DG.gate(dmaps[img], row_mask[n], **kw)
            wds = XG.frame_words(keep)
            expect[PAD + ooffs[n]:PAD + ooffs[n] + len(wds)] = wds
        else:
            want_counts[n] = REFUSED
    got_counts, got_levels = np_(counts), np_(levels)
    for n, (img, bad) in enumerate(rows):
        assert got_counts[n].tolist() == want_counts[n].tolist(), (n, bad, got_counts[n])
        np.testing.assert_array_equal(got_levels[n], want_levels[n], err_msg=f"levels of row {n} ({bad})")
    changed = np.flatnonzero(u32(out) != expect)
    assert not len(changed), (changed[:8] - PAD, [(n, bad) for n, (_, bad) in enumerate(rows) if bad])
    np.testing.assert_array_equal(u32(d.bits_all), inbuf)
    np.testing.assert_array_equal(np_(depth_all).view(np.uint32), dbuf.view(np.uint32))
    assert len(c.good) == 6 and all(0 < want_counts[n, 2] < want_counts[n, 0] for n in c.good)
    assert {bad for _, bad in rows} >= set(FR.INDEX_FAULTS + FR.OFFSET_FAULTS + [FR.END_FAULT] + [f for f, _ in FR.FRAME_FAULTS])
    # every good row equals the call made without the bad rows
    out2, counts2, levels2 = fresh(len(c.good))
    run(c.good, out2, counts2, levels2)
    np.testing.assert_array_equal(u32(out2), expect)                             # (the good rows keep their slots)
    np.testing.assert_array_equal(np_(counts2), want_counts[c.good])
    np.testing.assert_array_equal(np_(levels2), want_levels[c.good])
    # the statistics-only call makes the same decisions, but for the rows whose only fault lies in the output
    _, counts1, _ = fresh(B)
    run(range(B), None, counts1, None, with_out=False)
    got1 = np_(counts1)
    for n, (img, bad) in enumerate(rows):
        if bad is None:
            assert got1[n].tolist() == want_counts[n].tolist(), n
        elif "output" not in bad:
            assert got1[n].tolist() == REFUSED, (n, bad)
        else:
            assert got1[n, 0] > 0, (n, bad)                                      # a conforming input: gated
    # a depth buffer one element short of the last image's plane: that image's rows are refused, the others are unchanged
    out3, counts3, levels3 = fresh(len(c.good))
    run(c.good, out3, counts3, levels3, elems=delems - 1)
    expect3 = expect.copy()
    want3, short = want_counts[c.good].copy(), 0
    for j, n in enumerate(c.good):
        if rows[n][0] == 2:
            want3[j] = REFUSED
            expect3[PAD + ooffs[n]:PAD + ooffs[n] + XG.plane_words(*good[2])] = SENTINEL
            short += 1
    assert short == 2
    np.testing.assert_array_equal(np_(counts3), want3)
    np.testing.assert_array_equal(u32(out3), expect3)
    assert np.isnan(np_(levels3)[(want3[:, 0] == -2)]).all()


def test_no_image_refuses_every_row_and_empty_batches(la):
    """P == 0 with B > 0: no frame row is ever addressed, every row says refused and no plane word is written; B == 0: empty results"""
    import torch

    from labelany3d_amd.frames import _table_fields, frame_table

    B = 3
    bits = torch.zeros(64, dtype=torch.int32, device="cuda")
    depth = torch.ones(64, dtype=torch.float32, device="cuda")
    out = torch.full((256,), SENTINEL, dtype=torch.int32, device="cuda")
    offs = torch.arange(B, dtype=torch.int64, device="cuda") * 16
    counts = torch.full((B, 3), -7, dtype=torch.int32, device="cuda")
    levels = torch.full((B, 3), -7.0, dtype=torch.float32, device="cuda")
    c_gate(depth, 64, None, 0, 8, 32, torch.zeros(B, dtype=torch.int32, device="cuda"), B, bits, 64, offs, out, 256, offs, counts, levels)
    assert np_(counts).tolist() == [REFUSED] * B and (u32(out) == SENTINEL).all() and np.isnan(np_(levels)).all()

    def empty(sizes):
        t = frame_table(sizes)
        pf = la.PackedFrames(torch.zeros(4, dtype=torch.float32, device="cuda"), *_table_fields(t, sizes, torch.device("cuda", 0)))
        z = torch.zeros(0, dtype=torch.int32, device="cuda")
        return pf, la.FrameBits(torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"), z, z, t, pf.H, pf.W)

    for pf, fb in (empty(list(XG.SIZES)), empty([])):                            # B = 0; P = 0 with B = 0
        res, stats = la.gate_depth_bits_frames(pf, fb, return_stats=True)
        assert tuple(stats.counts.shape) == tuple(stats.levels.shape) == (0, 3) and res.area.numel() == 0 and res.offsets is fb.offsets
        assert tuple(la.depth_gate_stats_frames(pf, fb).counts.shape) == (0, 3)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------
# 7. in place, statistics only, two runs
# ------------------------------------------------------------------------------------------
def test_in_place_statistics_only_and_two_runs(la):
    import torch

    pf, fb = mixed(la)
    before = u32(fb.bits).copy()
    kw = dict(k=1.0, min_band=0.05)
    want = XG.expected(2)
    assert DG.PARAMS[2] == kw
    out = torch.full((fb.bits.numel() + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    first, s1 = la.gate_depth_bits_frames(pf, fb, out=out, return_stats=True, **kw)
    one = u32(out).copy(), np_(s1.counts).copy(), np_(s1.levels).copy()
    assert first.bits is out
    check(first, s1, want, "first", fb)
    out.fill_(SENTINEL)
    second, s2 = la.gate_depth_bits_frames(pf, fb, out=out, return_stats=True, **kw)
    np.testing.assert_array_equal(u32(out), one[0])                              # two runs: bit-identical, sentinels between the planes included
    np.testing.assert_array_equal(np_(s2.counts), one[1])
    np.testing.assert_array_equal(np_(s2.levels).view(np.uint32), one[2].view(np.uint32))
    only = la.depth_gate_stats_frames(pf, fb, **kw)                              # no plane written, the same statistics
    assert isinstance(only, la.DepthGateStats)
    np.testing.assert_array_equal(np_(only.counts), one[1])
    np.testing.assert_array_equal(np_(only.levels).view(np.uint32), one[2].view(np.uint32))
    np.testing.assert_array_equal(u32(fb.bits), before)
    alone = la.gate_depth_bits_frames(pf, fb, **kw)                              # without return_stats: the planes alone
    assert isinstance(alone, la.FrameBits)
    check(alone, None, want, "alone", fb)
    work = fb._replace(bits=fb.bits.clone())
    res, s3 = la.gate_depth_bits_frames(pf, work, out=work.bits, return_stats=True, **kw)   # in place
    assert res.bits is work.bits
    check(res, s3, want, "in place", work)
    with pytest.raises(ValueError, match="overlaps"):
        la.gate_depth_bits_frames(pf, fb, out=fb.bits[4:])
    with pytest.raises(ValueError, match="overlaps"):
        la.gate_depth_bits_frames(pf, fb, out=fb.bits[:-4])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    res, st = la.gate_depth_bits_frames(pf, fb, stream=side, return_stats=True, **kw)
    side.synchronize()
    check(res, st, want, "side stream", fb)


# ------------------------------------------------------------------------------------------
# 8. one call captured into a graph
# ------------------------------------------------------------------------------------------
def test_one_captured_call_replayed_on_changed_planes_and_depths(la):
    import torch

    pf0, fb0 = mixed(la)
    P = len(XG.SIZES)
    pf = pf0._replace(depth=torch.zeros_like(pf0.depth))
    fb = fb0._replace(bits=torch.zeros_like(fb0.bits))
    out = torch.zeros(fb.bits.numel(), dtype=torch.int32, device="cuda")
    kw = dict(k=1.0, min_band=0.05)
    side = torch.cuda.Stream()
    gr = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        la.gate_depth_bits_frames(pf, fb, out=out, return_stats=True, **kw)      # (warm-up)
        side.synchronize()
        with torch.cuda.graph(gr, stream=side):
            res, stats = la.gate_depth_bits_frames(pf, fb, out=out, return_stats=True, **kw)
    # the second set: the two rows of every image swapped, over the float16-rounded depth
    swapped = [XG.masks()[b ^ 1] for b in range(XG.B)]
    other = XG.upconverted(D16.VARIANTS[0])
    sets = (("g1", XG.depth_maps(), XG.masks(), pf0.depth, fb0.bits),
            ("g2", other, swapped, packed_depth(la, "mixed f16 as f32", other).depth, packed_bits(la, "mixed swapped", swapped, XG.IMAGE_INDEX, P)[1].bits))
    for tag, maps, row_masks, dd, bb in sets:
        pf.depth.copy_(dd)                                                       # changed planes and depths in the captured buffers
        fb.bits.copy_(bb)
        out.fill_(SENTINEL)
        stats.counts.fill_(-7)
        stats.levels.fill_(-7.0)
        res.area.fill_(-7)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        check(res, stats, XG.gate_rows(maps, row_masks, XG.IMAGE_INDEX, **kw), tag)
    assert not np.array_equal(XG.gate_rows(other, swapped, XG.IMAGE_INDEX, **kw)[1], XG.expected(2)[1])


# ------------------------------------------------------------------------------------------
# 9. the fit downstream
# ------------------------------------------------------------------------------------------
def fit_scene():
    """blob masks of the mixed sizes over tilted surfaces with a far strip and fill values: the gate changes them, the fit takes them"""
    rs = np.random.RandomState(91)
    maps = []
    for h, w in XG.SIZES:
        d = DG.smooth(rs, h, w)
        d[:, w - max(w // 8, 1):] = np.float32(7.5)
        d.reshape(-1)[rs.permutation(h * w)[:max(h * w // 50, 1)]] = DG.FILL
        maps.append(d)
    return maps, OF.planes(7, 1)


@pytest.mark.parametrize("variant", [None, D16.VARIANTS[1]], ids=["PackedFrames", "PackedFrames16-u16"])
def test_the_fit_downstream_takes_the_gated_planes(la, variant):
    """fit_instances_frames_bits on the gated planes = the same fit on pack_mask_bits_frames of the oracle's keep: records, statuses, aux"""
    maps, row_masks = fit_scene()
    P = len(XG.SIZES)
    if variant is not None:
        store = [D16.quantise(d, variant[0], variant[1]) for d in maps]
        maps = [D16.upconvert(x, variant[1], variant[2]) for x in store]
        pf = packed_depth(la, f"fit {variant}", store, variant)
    else:
        pf = packed_depth(la, "fit f32", maps)
    fb = packed_bits(la, "fit", row_masks, XG.IMAGE_INDEX, P)[1]
    keeps, counts, _ = XG.gate_rows(maps, row_masks, XG.IMAGE_INDEX)
    assert (counts[:, 2] < counts[:, 0]).sum() >= 12
    gated = la.gate_depth_bits_frames(pf, fb)
    theirs = packed_bits(la, f"fit keep {variant}", keeps, XG.IMAGE_INDEX, P)[1]
    K = np.stack([IC.cameras(1, h, w)[0] for h, w in XG.SIZES])
    got = la.fit_instances_frames_bits(pf, gated, K)
    want = la.fit_instances_frames_bits(pf, theirs, K)
    np.testing.assert_array_equal(np_(got["status"]), np_(want["status"]))
    np.testing.assert_array_equal(np_(got["boxes"]), np_(want["boxes"]))         # (NaN == NaN in the same place)
    np.testing.assert_array_equal(np_(got["aux"]), np_(want["aux"]))
    assert (np_(got["status"]) == 0).sum() >= 12 and (np_(want["status"]) == 0).sum() >= 12, np_(got["status"])


# ------------------------------------------------------------------------------------------
# 10. the case the feature exists for
# ------------------------------------------------------------------------------------------
def test_the_case_the_feature_exists_for(la):
    """the 48 x 64 instance at 2 m +- 5 cm whose mask bleeds onto the wall at 7.5 m and holds one 10000.0 pixel, and a copy cropped to
    33 x 47, in ONE call: ungated the fitted boxes are kilometres deep, gated with the defaults they are the object's"""
    depth, mask = DG.scene()
    maps, row_masks = [depth, depth[:33, :47].copy()], [mask, mask[:33, :47].copy()]
    ii = np.arange(2)
    pf = packed_depth(la, "scene", maps)
    fb = packed_bits(la, "scene", row_masks, ii, 2)[1]
    K = np.stack([np.array([[120.0, 0.0, w / 2.0], [0.0, 120.0, h / 2.0], [0.0, 0.0, 1.0]]) for h, w in ((48, 64), (33, 47))])

    def depth_extent(bits):
        fit = la.fit_instances_frames_bits(pf, bits, K)
        assert np_(fit["status"]).tolist() == [0, 0]
        z = np_(la.unpack_boxes(fit["boxes"])["bbox3D_cam"])[:, :, 2]
        return z.max(1) - z.min(1)

    assert (depth_extent(fb) > 1000).all()
    gated, stats = la.gate_depth_bits_frames(pf, fb, return_stats=True)
    check(gated, stats, XG.gate_rows(maps, row_masks, ii), "scene", fb)
    assert np_(stats.counts)[0].tolist() == [1280, 1280, 1151] and np_(stats.counts)[1, 2] < np_(stats.counts)[1, 0]
    assert (depth_extent(gated) < 0.5).all()
