"""GPU tests of the frames form of connected components on bit planes (include/la3d.h "connected components on bit planes",
la3d_components_bits_frames; ``components_bits_frames``, ``largest_component_bits_frames``, ``drop_islands_bits_frames``,
``components_stats_frames``): the planes of images of different sizes labelled in ONE call, planes, statistics and tables exact
against the NumPy restatement of the rule (tests/components_cases.py) and bit for bit against the uniform ``components_bits``;
exactly the plane's words written; the rows the device refuses; capacity; the statistics-only call; ``out`` reuse; shared offsets;
one captured call; the consumers.  Nothing here imports SciPy."""
import ctypes as C

import numpy as np
import pytest

from . import components_cases as CC
from . import components_frames_cases as XC
from . import frames_fault_rows as FR
from . import instance_points_cases as IC

pytestmark = pytest.mark.gpu

SENTINEL = CC.SENTINEL
REFUSED = XC.REFUSED
ROWS = XC.TABLE_ROWS
MAX_RUNS = 4096                                    # above every case (MAX_CASE_RUNS = 3500): 16 KiB of LDS per workgroup


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


_PACKED = {}


def packed(la, masks=None, sizes=XC.SIZES, per_image=XC.PER_IMAGE, key="cases"):
    """planes in image order, per_image of each -> (PackedMasks, FrameBits); the PackedMasks is the ``frames`` of the calls.  Packed
    once per key and shared: no test writes into either"""
    if key not in _PACKED:
        pm = la.pack_mask_frames(XC.stacks(XC.planes() if masks is None else masks, sizes, per_image))
        _PACKED[key] = pm, la.pack_mask_bits_frames(pm)
    return _PACKED[key]


def plane_of(bits, offsets, n, h, w):
    o = int(np_(offsets)[n])
    return u32(bits)[o:o + XC.plane_words(h, w)]


def check(res, stats, tab, want, tag, fb=None):
    """res: the FrameBits of a call; want: (outs, stats, tables) of XC.expected"""
    outs, want_stats, want_tab = want
    assert len(np_(res.offsets)) == len(outs), tag
    for n, m in enumerate(outs):
        np.testing.assert_array_equal(plane_of(res.bits, res.offsets, n, *m.shape), XC.frame_words(m), err_msg=f"{tag}[{n}] {m.shape}")
    if stats is not None:
        assert tuple(stats.shape) == (len(outs), 8) and not stats.dtype.is_floating_point, tag
        np.testing.assert_array_equal(np_(stats), want_stats, err_msg=f"{tag} stats")
    if tab is not None:
        np.testing.assert_array_equal(np_(tab), want_tab, err_msg=f"{tag} table")
    np.testing.assert_array_equal(np_(res.area), np.maximum(want_stats[:, 3], 0), err_msg=f"{tag} area")
    if fb is not None:
        assert res.offsets is fb.offsets and res.image_index is fb.image_index and res.table is fb.table and (res.H, res.W) == (fb.H, fb.W), tag


def ptr(t, words=0):
    return C.c_void_p(t.data_ptr() + 4 * words)


def workspace(B, H, max_runs, fill=None):
    import torch

    from labelany3d_amd import _lib

    n = max(int(_lib.lib.la3d_components_workspace_bytes(B, H, max_runs)) // 4, 1)
    return torch.empty(n, dtype=torch.int32, device="cuda") if fill is None else torch.full((n,), fill, dtype=torch.int32, device="cuda")


def c_comp(bits, bits_words, offs, table, P, H, W, ii, B, out, out_words, ooffs, stats, comps, conn=8, min_area=0, largest=False,
           max_runs=MAX_RUNS, rows=ROWS, ws=None, stream=None):
    """the C entry on device tensors or ready c_void_p values"""
    import torch

    from labelany3d_amd import _lib

    ws = workspace(B, H, max_runs) if ws is None else ws
    p = [None if x is None else (x.value if isinstance(x, C.c_void_p) else x.data_ptr()) for x in (bits, offs, table, ii, out, ooffs, stats, comps, ws)]
    st = torch.cuda.current_stream() if stream is None else stream
    a = _lib.ComponentsFramesArgs(struct_size=C.sizeof(_lib.ComponentsFramesArgs), B=B, P=P, H=H, W=W, connectivity=conn, min_area=min_area,
                                  largest=int(largest), max_runs=max_runs, max_components=rows if comps is not None else 0,
                                  bits=p[0], bits_words=bits_words, bits_offsets=p[1], frames=p[2], image_index=p[3],
                                  out_bits=p[4], out_words=out_words, out_offsets=p[5], stats=p[6], components=p[7], workspace=p[8],
                                  stream=st.cuda_stream)
    rc = _lib.lib.la3d_components_bits_frames(C.byref(a))
    assert rc == 0, _lib.lib.la3d_last_error()
    return ws


# ------------------------------------------------------------------------------------------
# 1. the mixed list, exact
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_area,largest", XC.RULES4)
@pytest.mark.parametrize("conn", XC.CONNECTIVITIES)
def test_mixed_sizes_exact(la, conn, min_area, largest):
    """24 planes of 12 sizes in one call: every plane, statistics row and table is the restatement's"""
    pm, fb = packed(la)
    res, stats, tab = la.components_bits_frames(pm, fb, min_area=min_area, largest=largest, connectivity=conn, max_components=ROWS,
                                                max_runs=MAX_RUNS)
    assert isinstance(res, la.FrameBits) and tuple(tab.shape) == (24, ROWS, 5)
    check(res, stats, tab, XC.expected(conn, min_area, largest), f"conn={conn} rule={(min_area, largest)}", fb)


# ------------------------------------------------------------------------------------------
# 2. garbage in the bits that are not image; exactly the plane's words
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", XC.CONNECTIVITIES)
def test_garbage_in_padding_and_between_planes_and_sentinels_around_every_output(la, conn):
    import torch

    pm, fb = packed(la)
    masks = XC.planes()
    B = len(masks)
    offs = np_(fb.offsets)
    dirty = np.random.RandomState(9).randint(0, 2 ** 32, fb.bits.numel(), dtype=np.uint64).astype(np.uint32)    # garbage between the planes
    set_pad = 0
    for n, m in enumerate(masks):
        h, w = m.shape
        pad = np.ones((h, CC.padded(w)), bool)
        pad[:, :w] = m                                                           # every padding column set
        wds = CC.words(pad, CC.padded(w))
        set_pad += int(np.bitwise_xor(wds, XC.frame_words(m)).any())
        dirty[offs[n]:offs[n] + len(wds)] = wds
    assert set_pad >= 12 and (dirty != u32(fb.bits)).any()
    src = torch.as_tensor(dirty.view(np.int32), device="cuda")
    words = [XC.plane_words(*m.shape) for m in masks]
    ooffs, at = [], 8
    for n in range(B):                                                           # hand-made offsets: multiples of 4, gaps between planes
        ooffs.append(at)
        at += (words[n] + 3) // 4 * 4 + 4 * (1 + n % 3)
    ooffs_d = torch.as_tensor(np.array(ooffs, np.int64), device="cuda")
    for min_area, largest in XC.RULES4:
        outs, want_stats, want_tab = XC.expected(conn, min_area, largest)
        out = torch.full((at + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        stats = torch.full((B, 8), -7, dtype=torch.int32, device="cuda")
        tab = torch.full((B, ROWS, 5), -7, dtype=torch.int32, device="cuda")
        c_comp(src, src.numel(), fb.offsets, pm.table, len(XC.SIZES), pm.H, pm.W, fb.image_index, B, out, out.numel(), ooffs_d, stats, tab,
               conn=conn, min_area=min_area, largest=largest)
        expect = np.full(at + 8, SENTINEL, np.uint32)
        for n, m in enumerate(outs):
            expect[ooffs[n]:ooffs[n] + words[n]] = XC.frame_words(m)             # (padding columns zero)
        np.testing.assert_array_equal(u32(out), expect, err_msg=f"rule={(min_area, largest)}")
        np.testing.assert_array_equal(np_(stats), want_stats)
        np.testing.assert_array_equal(np_(tab), want_tab)
    np.testing.assert_array_equal(u32(src), dirty)


# ------------------------------------------------------------------------------------------
# 3. a uniform-size FrameBits equals components_bits
# ------------------------------------------------------------------------------------------
def uniform_equal(la, masks, key, rules, rows, max_runs):
    import torch

    h, w = masks[0].shape
    B = len(masks)
    pm, fb = packed(la, list(masks), [(h, w)], B, key=key)
    one = la.pack_mask_bits(torch.as_tensor(np.stack(masks).astype(np.uint8), device="cuda"), frame_pad=True)
    nw = XC.plane_words(h, w)
    assert (one.H, one.W, one.frame_width) == (h, CC.padded(w), w)
    changed = 0
    for conn, min_area, largest in rules:
        res, stats, tab = la.components_bits_frames(pm, fb, min_area=min_area, largest=largest, connectivity=conn, max_components=rows, max_runs=max_runs)
        mb, st, tb = la.components_bits(one, min_area=min_area, largest=largest, connectivity=conn, max_components=rows, max_runs=max_runs)
        for n in range(B):
            np.testing.assert_array_equal(plane_of(res.bits, res.offsets, n, h, w), u32(mb.bits)[n, :nw], err_msg=f"{key} plane {n} {(conn, min_area, largest)}")
        np.testing.assert_array_equal(np_(stats), np_(st))
        np.testing.assert_array_equal(np_(tab), np_(tb))
        assert (np_(st)[:, 0] > 0).all()
        changed += int((np_(st)[:, 3] < np_(st)[:, 2]).any())
    assert changed


def test_uniform_sizes_equal_components_bits_33x47(la):
    masks = list(CC.fixture_planes()[0])
    uniform_equal(la, masks, "u33x47", [(c, a, l) for c in (4, 8) for a, l in XC.RULES4], ROWS, 2048)


def test_uniform_sizes_equal_components_bits_480x640(la):
    """three planes of 6.3 - 6.5 k runs at the default max_runs: parent in 64 KiB of LDS, rows of 20 words"""
    uniform_equal(la, list(CC.big_planes()), "u480x640", [(8, 0, True), (4, CC.MIN_AREA, False)], CC.TABLE_ROWS, 16384)


# ------------------------------------------------------------------------------------------
# 4. refused rows
# ------------------------------------------------------------------------------------------
def test_refused_rows_write_nothing_and_say_so(la):
    """One bad value per refused row - the shared case table (tests/frames_fault_rows.py) and the faults of the output, which are this
    entry's own; every address a defect would form from it lies inside this test's own allocations (the table, the input and the
    output have pad in front and behind), so a defect shows as a changed word, never as a fault."""
    import torch

    conn, min_area, largest = 8, CC.MIN_AREA, False
    rs = np.random.RandomState(4)
    SLOT, PAD = FR.SLOT, FR.PAD                                                  # slots of 128 words hold every plane, bad rows included
    c = FR.case(end_check=True, extra=[(1, "output offset 6"), (2, "output offset -4"), (0, "output plane ends one word past out_words")])
    rows, B, P, H, W, good = c.rows, c.B, c.P, c.H, c.W, FR.GOOD
    bits_words, out_words = c.words, B * SLOT + 1
    ioffs, ooffs = c.offsets, np.arange(B, dtype=np.int64) * SLOT
    for n, (img, bad) in enumerate(rows):
        if bad == "output offset 6":
            ooffs[n] += 6
        elif bad == "output offset -4":
            ooffs[n] = -4
        elif bad == "output plane ends one word past out_words":
            ooffs[n] = out_words - XC.plane_words(*good[img]) + 1
            assert ooffs[n] % 4 == 0 and ooffs[n] >= 0
    named = {n: (f"refusal{n}", CC.blob_plane(rs, *good[rows[n][0]], noise=0.04)) for n in c.good}
    inbuf = FR.input_words(c, rs, lambda n, h, w: XC.frame_words(named[n][1]))   # garbage wherever no plane lies
    d = FR.on_device(c, inbuf)
    inp, table, ii = d.bits_all, d.table_all, d.image_index
    out = torch.full((PAD + out_words + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    stats = torch.full((B, 8), -7, dtype=torch.int32, device="cuda")
    tab = torch.full((B, ROWS, 5), -7, dtype=torch.int32, device="cuda")
    ioffs_d, ooffs_d = torch.as_tensor(ioffs, device="cuda"), torch.as_tensor(ooffs, device="cuda")
    frames = C.c_void_p(table.data_ptr() + 24)
    c_comp(ptr(inp, PAD), bits_words, ioffs_d, frames, P, H, W, ii, B, ptr(out, PAD), out_words, ooffs_d, stats, tab,
           conn=conn, min_area=min_area, largest=largest, max_runs=2048)
    expect = np.full(PAD + out_words + PAD, SENTINEL, np.uint32)
    want_stats, want_tab = [], []
    for n, (img, bad) in enumerate(rows):
        if bad is None:
            (o,), st, tb = XC.expected(conn, min_area, largest, named=[named[n]])
            wds = XC.frame_words(o)
            expect[PAD + ooffs[n]:PAD + ooffs[n] + len(wds)] = wds
            want_stats.append(st[0].tolist()); want_tab.append(tb[0])
        else:
            want_stats.append(REFUSED); want_tab.append(np.zeros((ROWS, 5), np.int32))
    got, got_tab = np_(stats).tolist(), np_(tab)
    for n, (img, bad) in enumerate(rows):
        assert got[n] == want_stats[n], (n, bad, got[n])
        np.testing.assert_array_equal(got_tab[n], want_tab[n], err_msg=f"table of row {n} ({bad})")
    changed = np.flatnonzero(u32(out) != expect)
    assert not len(changed), (changed[:8] - PAD, [(n, bad) for n, (_, bad) in enumerate(rows) if bad])
    np.testing.assert_array_equal(u32(inp), inbuf)
    assert sum(bad is None for _, bad in rows) == 6 and all(want_stats[n][3] > 0 for n in named)
    assert {bad for _, bad in rows} >= set(FR.INDEX_FAULTS + FR.OFFSET_FAULTS + [FR.END_FAULT] + [f for f, _ in FR.FRAME_FAULTS])
    # the statistics-only call makes the same decisions, but for the rows whose only fault lies in the output
    stats1 = torch.full((B, 8), -7, dtype=torch.int32, device="cuda")
    c_comp(ptr(inp, PAD), bits_words, ioffs_d, frames, P, H, W, ii, B, None, 0, None, stats1, None, conn=conn, min_area=min_area,
           largest=largest, max_runs=2048)
    got1 = np_(stats1).tolist()
    for n, (img, bad) in enumerate(rows):
        if bad is None:
            assert got1[n] == want_stats[n], n
        elif "output" not in bad:
            assert got1[n] == REFUSED, (n, bad)
        else:
            assert got1[n][0] >= 0, (n, bad)                                     # a conforming input: labelled
    assert (u32(out) == expect).all()


def test_no_image_refuses_every_row(la):
    """P == 0 with B > 0: no frame row is ever addressed; every statistics row says refused, the table rows are zero and no plane
    word is written"""
    import torch

    B = 3
    bits = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.full((256,), SENTINEL, dtype=torch.int32, device="cuda")
    offs = torch.arange(B, dtype=torch.int64, device="cuda") * 16
    stats = torch.full((B, 8), -7, dtype=torch.int32, device="cuda")
    tab = torch.full((B, ROWS, 5), -7, dtype=torch.int32, device="cuda")
    c_comp(bits, 64, offs, None, 0, 8, 32, torch.zeros(B, dtype=torch.int32, device="cuda"), B, out, 256, offs, stats, tab, max_runs=64)
    assert np_(stats).tolist() == [REFUSED] * B and (u32(out) == SENTINEL).all() and not np_(tab).any()


# ------------------------------------------------------------------------------------------
# 5. capacity
# ------------------------------------------------------------------------------------------
def test_max_runs_at_the_edge(la):
    """max_runs equal to the most runs any row has: every row passes; one less: that row alone gets -1, runs and an all-zero plane"""
    pm, fb = packed(la)
    runs = [CC.count_runs(m) for m in XC.planes()]
    R = max(runs)
    assert runs.count(R) == 1 and R > 512
    for max_runs, over in ((R, 0), (R - 1, 1)):
        res, stats, tab = la.components_bits_frames(pm, fb, min_area=2, connectivity=8, max_components=ROWS, max_runs=max_runs)
        want = XC.expected(8, 2, False, max_runs=max_runs)
        assert (want[1][:, 0] == -1).sum() == over
        check(res, stats, tab, want, f"max_runs={max_runs}", fb)
    n = runs.index(R)
    assert np_(stats)[n].tolist() == [-1, R, 0, 0, 0, 0, 0, 0] and int(np_(res.area)[n]) == 0
    st = np_(la.components_stats_frames(pm, fb, max_runs=1))
    for n, r in enumerate(runs):
        assert (st[n, 0] == -1 and st[n, 1] == r) if r > 1 else st[n, 0] == r, n


# ------------------------------------------------------------------------------------------
# 6. forms of the call
# ------------------------------------------------------------------------------------------
def test_statistics_only_writes_nothing_and_out_is_reused(la):
    import torch

    pm, fb = packed(la)
    before = u32(fb.bits).copy()
    want = XC.expected(4, CC.MIN_AREA, True)
    st, tb = la.components_stats_frames(pm, fb, min_area=CC.MIN_AREA, largest=True, connectivity=4, max_components=ROWS, max_runs=MAX_RUNS)
    np.testing.assert_array_equal(np_(st), want[1])
    np.testing.assert_array_equal(np_(tb), want[2])
    st = la.components_stats_frames(pm, fb, min_area=CC.MIN_AREA, largest=True, connectivity=4, max_runs=MAX_RUNS)
    np.testing.assert_array_equal(np_(st), want[1])
    np.testing.assert_array_equal(u32(fb.bits), before)
    # out=: one buffer filled by three calls in turn, each leaving what lies between and behind the planes alone
    n = fb.bits.numel()
    out = torch.full((n + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    words = np.zeros(n + 8, bool)
    for b, m in enumerate(XC.planes()):
        o = int(np_(fb.offsets)[b])
        words[o:o + XC.plane_words(*m.shape)] = True
    for tag, fn, rule in (("largest", lambda **kw: la.largest_component_bits_frames(pm, fb, **kw), (8, 0, True)),
                          ("islands", lambda **kw: la.drop_islands_bits_frames(pm, fb, CC.MIN_AREA, connectivity=4, **kw), (4, CC.MIN_AREA, False)),
                          ("largest again", lambda **kw: la.largest_component_bits_frames(pm, fb, **kw), (8, 0, True))):
        res = fn(out=out, max_runs=MAX_RUNS)
        assert isinstance(res, la.FrameBits) and res.bits is out
        check(res, None, None, XC.expected(*rule), tag, fb)
        assert (u32(out)[~words] == SENTINEL).all(), tag
        res2, st2 = fn(return_stats=True, max_runs=MAX_RUNS)
        check(res2, st2, None, XC.expected(*rule), tag + " fresh", fb)
    with pytest.raises(ValueError, match="overlaps"):
        la.components_bits_frames(pm, fb, out=fb.bits)
    with pytest.raises(ValueError, match="out must be"):
        la.components_bits_frames(pm, fb, out=out[:64])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    res, st = la.components_bits_frames(pm, fb, min_area=3, stream=side, return_stats=True, max_runs=MAX_RUNS)
    side.synchronize()
    check(res, st, None, XC.expected(8, 3, False), "side stream", fb)


def test_out_offsets_may_be_the_pointer_given_as_bits_offsets(la):
    import torch

    pm, fb = packed(la)
    B = len(XC.planes())
    out = torch.full((fb.bits.numel(),), SENTINEL, dtype=torch.int32, device="cuda")
    stats = torch.full((B, 8), -7, dtype=torch.int32, device="cuda")
    c_comp(fb.bits, fb.bits.numel(), fb.offsets, pm.table, len(XC.SIZES), pm.H, pm.W, fb.image_index, B, out, out.numel(), fb.offsets, stats, None,
           conn=4, largest=True)
    want = XC.expected(4, 0, True)
    res = la.FrameBits(out, fb.offsets, fb.image_index, stats[:, 3].contiguous(), fb.table, fb.H, fb.W)
    check(res, stats, None, want, "shared offsets")
    # planes without statistics: the same words
    out2 = torch.full_like(out, SENTINEL)
    c_comp(fb.bits, fb.bits.numel(), fb.offsets, pm.table, len(XC.SIZES), pm.H, pm.W, fb.image_index, B, out2, out2.numel(), fb.offsets, None, None,
           conn=4, largest=True)
    np.testing.assert_array_equal(u32(out2), u32(out))


def test_empty_batches(la):
    import torch

    from labelany3d_amd.frames import _table_fields, frame_table

    def empty(sizes):
        grid = la.FrameGrid(*_table_fields(frame_table(sizes), sizes, torch.device("cuda", 0)))
        z = torch.zeros(0, dtype=torch.int32, device="cuda")
        return grid, la.FrameBits(torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"), z, z,
                                  grid.table_host, grid.H, grid.W)

    for frames, bits in (empty(list(XC.SIZES)), empty([])):                      # B = 0; P = 0 with B = 0
        res, stats, tab = la.components_bits_frames(frames, bits, max_components=3)
        assert tuple(stats.shape) == (0, 8) and tuple(tab.shape) == (0, 3, 5) and res.area.numel() == 0 and res.offsets is bits.offsets
        assert tuple(la.components_stats_frames(frames, bits).shape) == (0, 8)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------
# 7. one call captured into a graph
# ------------------------------------------------------------------------------------------
def test_one_call_captured_into_a_graph_and_replayed_once(la):
    import torch

    pm, fb = packed(la)
    B, P = len(XC.planes()), len(XC.SIZES)
    conn, min_area, largest = 8, CC.MIN_AREA, True
    src = fb.bits.clone()
    out = torch.zeros(fb.bits.numel(), dtype=torch.int32, device="cuda")
    stats = torch.zeros((B, 8), dtype=torch.int32, device="cuda")
    tab = torch.zeros((B, ROWS, 5), dtype=torch.int32, device="cuda")
    ws = workspace(B, pm.H, MAX_RUNS)

    def run(stream):
        c_comp(src, src.numel(), fb.offsets, pm.table, P, pm.H, pm.W, fb.image_index, B, out, out.numel(), fb.offsets, stats, tab, conn=conn,
               min_area=min_area, largest=largest, ws=ws, stream=stream)

    side = torch.cuda.Stream()
    gr = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        run(side)                                                                # (warm-up)
        side.synchronize()
        with torch.cuda.graph(gr, stream=side):
            run(torch.cuda.current_stream())
    direct = u32(out).copy(), np_(stats).copy(), np_(tab).copy()
    out.fill_(SENTINEL)
    stats.fill_(-7)
    tab.fill_(-7)
    ws.fill_(-1)
    torch.cuda.synchronize()
    gr.replay()
    torch.cuda.synchronize()
    res = la.FrameBits(out, fb.offsets, fb.image_index, stats[:, 3].contiguous(), fb.table, fb.H, fb.W)
    check(res, stats, tab, XC.expected(conn, min_area, largest), "replay")
    np.testing.assert_array_equal(np_(stats), direct[1])
    np.testing.assert_array_equal(np_(tab), direct[2])
    for n, m in enumerate(XC.planes()):
        o = int(np_(fb.offsets)[n])
        np.testing.assert_array_equal(u32(out)[o:o + XC.plane_words(*m.shape)], direct[0][o:o + XC.plane_words(*m.shape)])


# ------------------------------------------------------------------------------------------
# 8. consumers
# ------------------------------------------------------------------------------------------
def test_the_fit_of_the_largest_part_is_the_fit_of_the_restatements_planes(la):
    pm, fb = packed(la)
    want = XC.expected(8, 0, True)[0]
    rs = np.random.RandomState(2)
    pf = la.pack_frames([rs.uniform(0.5, 10.0, hw).astype(np.float32) for hw in XC.SIZES])
    K = np.stack([IC.cameras(1, h, w)[0] for h, w in XC.SIZES])
    res = la.largest_component_bits_frames(pm, fb, max_runs=MAX_RUNS)
    got = la.fit_instances_frames_bits(pf, res, K)
    ref = la.fit_instances_frames_bits(pf, packed(la, want, key="largest8")[1], K)
    np.testing.assert_array_equal(np_(got["status"]), np_(ref["status"]))
    np.testing.assert_array_equal(np_(got["boxes"]), np_(ref["boxes"]))          # (NaN == NaN in the same place)
    assert np.isfinite(np_(ref["boxes"])).any()
    assert any(not np.array_equal(w, m) for w, m in zip(want, XC.planes()))


def test_the_encoder_and_the_rectangles_accept_the_result(la):
    pm, fb = packed(la)
    want, want_stats, _ = XC.expected(4, CC.MIN_AREA, False)
    res, stats = la.drop_islands_bits_frames(pm, fb, CC.MIN_AREA, connectivity=4, max_runs=MAX_RUNS, return_stats=True)
    np.testing.assert_array_equal(np_(la.bits_rects_frames(pm, res)), want_stats[:, 3:])         # area, x, y, w, h of the output
    (counts, offsets), sizes = la.rle_encode_bits_frames(pm, res)
    objs = la.rle_objects((counts, offsets), sizes=sizes)
    assert len(objs) == len(want)
    for n, (o, m) in enumerate(zip(objs, want)):
        assert o["size"] == list(m.shape), n
        runs = np.asarray(o["counts"], np.int64)
        assert runs.sum() == m.size
        vals = np.zeros(len(runs), bool)
        vals[1::2] = True
        np.testing.assert_array_equal(np.repeat(vals, runs).reshape(m.shape[::-1]).T, m, err_msg=f"runs {n}")   # column-major
