"""GPU tests of connected components on bit planes (include/la3d.h "connected components on bit planes"; ``components_bits``,
``largest_component_bits``, ``drop_islands_bits``, ``components_stats``): the planes, statistics and tables against what SciPy gave
(tests/golden/g20_components.npz) and against the NumPy restatement of the rule (tests/components_cases.py), bit for bit and exact;
plane strides, sentinels and garbage in the bits that are not image; ``max_runs`` at the edge; tables shorter and longer than the
components; batch sizes; the statistics-only call and ``out`` reuse; the algebra; the consumers of the planes; the far island that the
feature exists for; one captured call.  Nothing here imports SciPy."""
import hashlib

import numpy as np
import pytest

from . import components_cases as CC
from . import instance_points_cases as IC

pytestmark = pytest.mark.gpu

SENTINEL = CC.SENTINEL
RULES4 = ((0, False), (CC.MIN_AREA, False), (0, True), (CC.MIN_AREA, True))


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


@pytest.fixture(scope="module")
def g():
    return CC.load_golden()


@pytest.fixture(scope="module")
def labelled():
    """the restatement's labelling of every case, made once per (case, connectivity) and shared"""
    memo = {}

    def of(name, mask, conn):
        key = (name, conn)
        if key not in memo:
            labels, n = CC.label(mask, conn)
            memo[key] = labels, n, CC.table_of(labels, n)
        return memo[key]

    return of


def np_(t):
    return t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()


def u32(t):
    return np_(t).view(np.uint32)


def planes_of(la, masks, pad=True):
    import torch

    return la.pack_mask_bits(torch.as_tensor(np.ascontiguousarray(masks).astype(np.uint8), device="cuda"), frame_pad=pad)


def expect(labelled, names, masks, conn, min_area, largest, rows):
    outs, stats, tabs = [], [], []
    for name, m in zip(names, masks):
        labels, n, table = labelled(name, m, conn)
        out, st = CC.choose(labels, n, table, min_area, largest)
        tab = np.zeros((rows, 5), np.int32)
        tab[:min(n, rows)] = table[:rows]
        outs.append(out); stats.append(st); tabs.append(tab)
    return outs, np.asarray(stats, np.int32).reshape(len(masks), 8), np.stack(tabs) if tabs else np.zeros((0, rows, 5), np.int32)


def check(res, src, want_out, want_stats, want_tab, tag):
    """res: what components_bits returned with a table; src: the input MaskBits"""
    mb, stats, tab = res
    assert (mb.H, mb.W, mb.frame_width) == (src.H, src.W, src.frame_width), tag
    nwords = (mb.H * mb.W + 31) // 32
    got = u32(mb.bits)
    assert got.shape[0] == len(want_out) and got.shape[1] >= nwords, tag
    np.testing.assert_array_equal(np_(stats), want_stats, err_msg=f"{tag} stats")
    np.testing.assert_array_equal(np_(tab), want_tab, err_msg=f"{tag} table")
    for b, m in enumerate(want_out):
        np.testing.assert_array_equal(got[b, :nwords], CC.words(m, mb.W), err_msg=f"{tag}[{b}]")


# ------------------------------------------------------------------------------------------
# 1. the fixture: SciPy's planes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,pad", [(0, False), (0, True), (1, True), (1, False), (2, True), (2, False)],
                         ids=["33x47", "33x47p", "96x224p", "96x224", "140x96p", "140x96"])
def test_fixture_planes_bit_for_bit(la, g, f, pad):
    H, W = CC.FIXTURE_FRAMES[f]
    ins = CC.unpack(g[f"in_{f}"], H, W)
    src = planes_of(la, ins, pad)
    seen = 0
    for conn in (4, 8):
        for r, (min_area, largest) in enumerate(CC.RULES):
            keys = [f"{f}_{p}_{conn}_{r}" for p in range(CC.FIXTURE_PLANES)]
            res = la.components_bits(src, min_area=min_area, largest=largest, connectivity=conn, max_components=CC.TABLE_ROWS, return_stats=True)
            outs = [CC.unpack(g[f"out_{k}"][None], H, W)[0] for k in keys]
            check(res, src, outs, np.stack([g[f"stats_{k}"] for k in keys]), np.stack([g[f"table_{k}"] for k in keys]), f"fixture {keys[0]}")
            seen += 1
    assert seen == 6


def test_fixture_big_planes(la, g):
    """three 480 x 640 planes of 6.3 - 6.5 k runs and 2 - 4 k components: statistics, the first 64 table rows, a hash of the output words"""
    H, W = CC.BIG_FRAME
    src = planes_of(la, CC.big_planes())
    for conn in (4, 8):
        for r, (min_area, largest) in enumerate(CC.RULES):
            keys = [f"big_{p}_{conn}_{r}" for p in range(len(CC.BIG_SEEDS))]
            mb, stats, tab = la.components_bits(src, min_area=min_area, largest=largest, connectivity=conn, max_components=CC.TABLE_ROWS)
            print(keys[0], np_(stats).tolist())
            np.testing.assert_array_equal(np_(stats), np.stack([g[f"stats_{k}"] for k in keys]), err_msg=keys[0])
            np.testing.assert_array_equal(np_(tab), np.stack([g[f"table_{k}"] for k in keys]), err_msg=keys[0])
            got = u32(mb.bits)
            for b, k in enumerate(keys):
                assert hashlib.sha256(got[b, :H * W // 32].astype("<u4").tobytes()).hexdigest() == bytes(g[f"sha_{k}"]).hex(), k
    # a bound below the planes' runs refuses all three, and says what they need
    stats = np_(la.components_stats(src, max_runs=6000))
    np.testing.assert_array_equal(stats[:, 0], -1)
    np.testing.assert_array_equal(stats[:, 1], g["big_runs"])
    assert not stats[:, 2:].any()


def test_long_strides_sentinels_and_garbage(la, g):
    """planes that lie further apart than their words, sentinel words between them left alone on the output side; pad columns and the
    bits past the plane full of garbage on the input side"""
    import torch

    f = 0
    H, W = CC.FIXTURE_FRAMES[f]
    ins = CC.unpack(g[f"in_{f}"], H, W)
    B = len(ins)
    for pad in (True, False):
        Ws = CC.padded(W) if pad else W
        nwords = (H * Ws + 31) // 32
        stride = nwords + 5
        bits = np.full((B, stride), SENTINEL, np.uint32)
        for b, m in enumerate(ins):
            dirty = np.ones((H, Ws), bool)                    # every bit that is not image: set
            dirty[:, :W] = m
            flat = np.concatenate([dirty.reshape(-1), np.ones((-H * Ws) % 32, bool)])
            bits[b, :nwords] = np.packbits(flat, bitorder="little").view(np.uint32)
        dev_in = torch.as_tensor(bits.view(np.int32), device="cuda")
        src = la.MaskBits(dev_in[:, :nwords + 2], H, Ws, W)                            # (rows dense, plane stride nwords + 5)
        assert src.bits.stride(0) == stride
        wide = torch.full((B, nwords + 7), SENTINEL, dtype=torch.int32, device="cuda")
        out = wide[:, :nwords]
        for conn, r in ((8, 2), (4, 1), (8, 0)):
            min_area, largest = CC.RULES[r]
            keys = [f"{f}_{p}_{conn}_{r}" for p in range(B)]
            res = la.components_bits(src, min_area=min_area, largest=largest, connectivity=conn, max_components=CC.TABLE_ROWS, out=out)
            assert res[0].bits is out
            outs = [CC.unpack(g[f"out_{k}"][None], H, W)[0] for k in keys]
            check(res, src, outs, np.stack([g[f"stats_{k}"] for k in keys]), np.stack([g[f"table_{k}"] for k in keys]), f"strides pad={pad} {keys[0]}")
            assert (u32(wide)[:, nwords:] == SENTINEL).all()
            assert (u32(dev_in)[:, nwords:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------
# 2. every pattern and random case against the restatement
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn,max_runs", [(8, 16384), (4, 16384), (8, 40000), (4, 3500)], ids=["c8", "c4", "c8-workspace-parent", "c4-3500"])
def test_every_case_against_the_restatement(la, labelled, conn, max_runs):
    """grouped by frame into one call per rule; both homes of the union-find (LDS up to 32768 runs, the workspace beyond)"""
    by_frame = {}
    for name, m in CC.all_cases():
        by_frame.setdefault(m.shape, []).append((name, m))
    rows = 24
    seen = 0
    for (H, W), group in by_frame.items():
        names, masks = [n for n, _ in group], np.stack([m for _, m in group])
        for pad in ((True, False) if W % 32 else (False,)):
            src = planes_of(la, masks, pad)
            for min_area, largest in RULES4:
                res = la.components_bits(src, min_area=min_area, largest=largest, connectivity=conn, max_components=rows, max_runs=max_runs)
                check(res, src, *expect(labelled, names, masks, conn, min_area, largest, rows), f"{names[0]}.. pad={pad} rule={(min_area, largest)}")
        seen += len(group)
    assert seen == len(CC.all_cases()) >= 130


# ------------------------------------------------------------------------------------------
# 3. capacity and tables
# ------------------------------------------------------------------------------------------
def test_max_runs_at_the_edge(la, labelled):
    import torch

    H, W = 61, 83
    rs = np.random.RandomState(5)
    masks = np.stack([CC.blob_plane(rs, H, W), rs.rand(H, W) < 0.45, CC.blob_plane(rs, H, W)])
    runs = [CC.count_runs(m) for m in masks]
    R = runs[1]
    assert R > max(runs[0], runs[2]) + 1 and R > 512
    names = [f"edge{i}" for i in range(3)]
    for pad in (True, False):
        src = planes_of(la, masks, pad)
        nwords = (H * src.W + 31) // 32
        for conn in (8, 4):
            outs, stats, tabs = expect(labelled, names, masks, conn, 2, False, 8)
            out = torch.full((3, nwords + 1), SENTINEL, dtype=torch.int32, device="cuda")
            check(la.components_bits(src, min_area=2, connectivity=conn, max_components=8, max_runs=R, out=out[:, :nwords]), src, outs, stats, tabs,
                  f"max_runs == runs pad={pad}")
            out.fill_(SENTINEL)
            outs[1] = np.zeros((H, W), bool)
            stats[1] = [-1, R, 0, 0, 0, 0, 0, 0]
            tabs[1] = 0
            check(la.components_bits(src, min_area=2, connectivity=conn, max_components=8, max_runs=R - 1, out=out[:, :nwords]), src, outs, stats, tabs,
                  f"max_runs == runs - 1 pad={pad}")
            assert (u32(out)[:, nwords] == SENTINEL).all()
    # the smallest bound: every plane with more than one run is refused, an empty plane and a one-run plane are not
    few = np.zeros((3, H, W), bool)
    few[1, 7, 3:80] = True
    few[2, 7, 3:80] = few[2, 9, 5] = True
    st = np_(la.components_stats(planes_of(la, few), max_runs=1))
    np.testing.assert_array_equal(st, [[0, 0, 0, 0, 0, 0, 0, 0], [1, 1, 77, 77, 3, 7, 77, 1], [-1, 2, 0, 0, 0, 0, 0, 0]])


def test_tables_shorter_and_longer_than_the_components(la, labelled):
    H, W = 33, 47
    rs = np.random.RandomState(8)
    masks = np.stack([rs.rand(H, W) < 0.2, CC.ring_with_dot(H, W), np.zeros((H, W), bool)])
    names = ["t0", "t1", "t2"]
    src = planes_of(la, masks)
    n0 = labelled("t0", masks[0], 8)[1]
    assert n0 > 40
    for rows in (1, 2, 7, n0 - 1, n0, n0 + 1, 3 * n0):
        outs, stats, tabs = expect(labelled, names, masks, 8, 3, False, rows)
        check(la.components_bits(src, min_area=3, max_components=rows), src, outs, stats, tabs, f"rows={rows}")
        st, tab = la.components_stats(src, min_area=3, max_components=rows)
        np.testing.assert_array_equal(np_(st), stats)
        np.testing.assert_array_equal(np_(tab), tabs)
        assert (stats[:, 0] > rows).tolist() == [n0 > rows, 2 > rows, False]          # n_components tells a truncated table


@pytest.mark.parametrize("B", [1, 2, 65, 257])
def test_batch_sizes(la, labelled, B):
    H, W = 40, 50
    rs = np.random.RandomState(3)
    base = np.stack([CC.blob_plane(rs, H, W, noise=0.05) for _ in range(5)])
    masks = base[np.arange(B) % 5].copy()
    masks[np.arange(B), np.arange(B) % H, :] ^= True            # no two planes alike
    names = [f"batch{b}" for b in range(B)]                     # (shared between the sizes: plane b is the same in each)
    src = planes_of(la, masks, False)
    for conn, min_area, largest in ((8, 0, True), (4, 5, False)):
        check(la.components_bits(src, min_area=min_area, largest=largest, connectivity=conn, max_components=4, max_runs=2048), src,
              *expect(labelled, names, masks, conn, min_area, largest, 4), f"B={B}")
    assert tuple(la.components_stats(planes_of(la, np.zeros((0, H, W), bool))).shape) == (0, 8)
    empty = la.components_bits(planes_of(la, np.zeros((0, H, W), bool)))
    assert tuple(empty.bits.shape)[0] == 0 and (empty.H, empty.frame_width) == (H, W)


# ------------------------------------------------------------------------------------------
# 4. forms of the call
# ------------------------------------------------------------------------------------------
def test_statistics_only_and_out_reuse(la, labelled):
    import torch

    H, W, B = 33, 47, 5
    rs = np.random.RandomState(12)
    a, b = (np.stack([CC.blob_plane(rs, H, W, noise=0.04) for _ in range(B)]) for _ in range(2))
    Ws = CC.padded(W)
    out = torch.full((B, (H * Ws + 31) // 32), SENTINEL, dtype=torch.int32, device="cuda")
    for tag, masks in (("a", a), ("b", b), ("a", a)):
        names = [f"reuse{tag}{i}" for i in range(B)]
        src = planes_of(la, masks)
        mb = la.largest_component_bits(src, out=out)
        assert isinstance(mb, la.MaskBits) and mb.bits is out
        outs, stats, _ = expect(labelled, names, masks, 8, 0, True, 0)
        for i, m in enumerate(outs):
            np.testing.assert_array_equal(u32(out)[i], CC.words(m, Ws), err_msg=f"out reuse {tag}[{i}]")
        mb2, st2 = la.largest_component_bits(src, return_stats=True)
        np.testing.assert_array_equal(np_(st2), stats)
        np.testing.assert_array_equal(u32(mb2.bits), u32(out))
        # out_bits = NULL: the same statistics, nothing else written
        np.testing.assert_array_equal(np_(la.components_stats(src, largest=True)), stats)
        outs4, stats4, _ = expect(labelled, names, masks, 4, 6, False, 0)
        mb4, st4 = la.drop_islands_bits(src, 6, connectivity=4, return_stats=True)
        np.testing.assert_array_equal(np_(st4), stats4)
        np.testing.assert_array_equal(np_(la.components_stats(src, min_area=6, connectivity=4)), stats4)
        for i, m in enumerate(outs4):
            np.testing.assert_array_equal(u32(mb4.bits)[i], CC.words(m, Ws))
    side = torch.cuda.Stream()
    src = planes_of(la, a)
    torch.cuda.synchronize()
    mb, st = la.components_bits(src, min_area=3, stream=side, return_stats=True)
    side.synchronize()
    outs, stats, _ = expect(labelled, [f"reusea{i}" for i in range(B)], a, 8, 3, False, 0)
    np.testing.assert_array_equal(np_(st), stats)


def test_algebra(la):
    rs = np.random.RandomState(77)
    H, W = 70, 100
    masks = rs.rand(8, H, W) < np.array([0.3, 0.41, 0.5, 0.59, 0.59, 0.7, 0.9, 1.0])[:, None, None]
    for pad in (True, False):
        src = planes_of(la, masks, pad)
        ident = la.drop_islands_bits(src, 0)
        np.testing.assert_array_equal(u32(ident.bits), u32(src.bits), err_msg="min_area = 0 is the identity")
        for conn in (4, 8):
            for min_area, largest in ((7, False), (0, True), (7, True), (10 ** 6, False)):
                mb, stats, tab = la.components_bits(src, min_area=min_area, largest=largest, connectivity=conn, max_components=4096)
                st, tab = np_(stats), np_(tab)
                assert not (u32(mb.bits) & ~u32(src.bits)).any(), "the output is a subset of the input"
                again, st2 = la.components_bits(mb, min_area=min_area, largest=largest, connectivity=conn, return_stats=True)
                np.testing.assert_array_equal(u32(again.bits), u32(mb.bits), err_msg="idempotent")
                np.testing.assert_array_equal(np_(st2)[:, 3:], st[:, 3:])
                np.testing.assert_array_equal(np_(st2)[:, 0], st[:, 1])         # what was kept is what is there
                assert (st[:, 0] <= 4096).all()
                areas = tab[:, :, 0]
                np.testing.assert_array_equal(areas.sum(1), st[:, 2])            # a complete table: the areas are the input
                if largest:
                    assert (st[:, 1] <= 1).all()
                    best = np.where(areas >= min_area, areas, 0).max(1)
                    np.testing.assert_array_equal(st[:, 3], best)
                else:
                    np.testing.assert_array_equal(st[:, 3], np.where(areas >= max(min_area, 1), areas, 0).sum(1))
                    np.testing.assert_array_equal(st[:, 1], (areas >= max(min_area, 1)).sum(1))
                np.testing.assert_array_equal(np_(la.mask_stats_bits(mb))[:, 0], st[:, 3])
                np.testing.assert_array_equal(np_(la.bits_rects(mb)), st[:, 3:])
                if min_area == 10 ** 6:
                    assert not u32(mb.bits).any() and not st[:, 3:].any()


# ------------------------------------------------------------------------------------------
# 5. consumers, and why the feature exists
# ------------------------------------------------------------------------------------------
def test_consumers_take_the_result(la, labelled):
    H, W, B = 96, 224, 6
    rs = np.random.RandomState(21)
    masks = np.stack([CC.blob_plane(rs, H, W) for _ in range(B)])
    want = np.stack(expect(labelled, [f"cons{i}" for i in range(B)], masks, 8, 0, True, 0)[0])
    assert want.any(axis=(1, 2)).all() and (want != masks).any(axis=(1, 2)).all()
    mb, stats = la.largest_component_bits(planes_of(la, masks), return_stats=True)
    np.testing.assert_array_equal(np_(la.rle_decode(la.rle_encode_bits(mb))).astype(bool), want)
    depth, K = IC.special_depth(B, H, W), IC.cameras(B, H, W)
    got = la.fit_instances_bits(depth, mb, K)
    ref = la.fit_instances_bits(depth, planes_of(la, want), K)
    np.testing.assert_array_equal(np_(got[1]), np_(ref[1]))
    np.testing.assert_array_equal(np_(got[0]), np_(ref[0]))                     # (NaN == NaN in the same place)
    assert np.isfinite(np_(ref[0])).any()
    ov = la.mask_overlap(mb, planes_of(la, masks))
    inter = np_(ov.matrix(0))
    np.testing.assert_array_equal(inter, (want[:, None] & masks[None]).sum(axis=(2, 3)))
    np.testing.assert_array_equal(np.diag(inter), np_(stats)[:, 3])             # the kept part lies inside its own input


def test_a_far_island_no_longer_stretches_the_box(la):
    """an object at 2 m and a small island three metres behind it, far away in the image: the fit of the raw mask spans both, the fit of
    ``largest_component_bits`` is the fit of the object alone, number for number"""
    H, W = 120, 160
    obj = np.zeros((H, W), bool)
    obj[40:80, 30:70] = True
    island = np.zeros((H, W), bool)
    island[100:104, 140:146] = True
    rs = np.random.RandomState(2)
    depth = np.full((H, W), 2.0, np.float32) + rs.uniform(0, 0.2, (H, W)).astype(np.float32)
    depth[island] += 3.0
    K = np.array([[150.0, 0, W / 2], [0, 150.0, H / 2], [0, 0, 1]])
    d3, K3 = np.stack([depth] * 3), np.stack([K] * 3)
    raw = planes_of(la, np.stack([obj | island, obj, obj | island]))
    clean, stats = la.largest_component_bits(raw, return_stats=True)
    np.testing.assert_array_equal(np_(stats)[:, :4], [[2, 1, 1624, 1600], [1, 1, 1600, 1600], [2, 1, 1624, 1600]])
    np.testing.assert_array_equal(np_(stats)[:, 4:], [[30, 40, 40, 40]] * 3)
    fit_raw = la.fit_instances_bits(d3, raw, K3)
    fit_clean = la.fit_instances_bits(d3, clean, K3)
    fit_alone = la.fit_instances_bits(d3, planes_of(la, np.stack([obj] * 3)), K3)
    rec_raw, rec_clean, rec_alone = np_(fit_raw[0]), np_(fit_clean[0]), np_(fit_alone[0])
    print("raw", rec_raw[0, :6].tolist(), "clean", rec_clean[0, :6].tolist())
    assert np.isfinite(rec_clean).all() and (np_(fit_clean[1]) == 0).all()
    np.testing.assert_array_equal(rec_clean, rec_alone)                          # the object alone, in every row
    np.testing.assert_array_equal(rec_raw[1], rec_alone[1])
    # the box spans its points: 24 pixels three metres behind the object stretch one side by metres and move the centre with it
    assert not np.array_equal(rec_raw[0], rec_alone[0]) and not np.array_equal(rec_raw[2], rec_alone[2])
    assert np.abs(rec_raw[0, 3:6] - rec_alone[0, 3:6]).max() > 1.0
    assert np.abs(rec_raw[0, 0:3] - rec_alone[0, 0:3]).max() > 0.5


# ------------------------------------------------------------------------------------------
# 6. one call captured into a graph
# ------------------------------------------------------------------------------------------
def test_one_call_captured_into_a_graph_and_replayed_on_changed_planes(la, labelled):
    import ctypes as C

    import torch

    from labelany3d_amd import _lib

    H, W, B, rows, max_runs = 33, 47, 8, 6, 1024
    rs = np.random.RandomState(41)
    first, second = (np.stack([CC.blob_plane(rs, H, W, noise=0.04) for _ in range(B)]) for _ in range(2))
    src = planes_of(la, first, False)
    nwords = (H * W + 31) // 32
    out = torch.zeros((B, nwords), dtype=torch.int32, device="cuda")
    stats = torch.zeros((B, 8), dtype=torch.int32, device="cuda")
    tab = torch.zeros((B, rows, 5), dtype=torch.int32, device="cuda")
    ws = torch.empty(_lib.lib.la3d_components_workspace_bytes(B, H, max_runs) // 4, dtype=torch.int32, device="cuda")

    def run(stream):
        a = _lib.ComponentsArgs(struct_size=C.sizeof(_lib.ComponentsArgs), B=B, H=H, W=W, frame_width=0, connectivity=8, min_area=3, largest=0,
                                max_runs=max_runs, max_components=rows, mask_bits=src.bits.data_ptr(), bits_plane_stride=src.bits.stride(0),
                                out_bits=out.data_ptr(), out_plane_stride=out.stride(0), stats=stats.data_ptr(), components=tab.data_ptr(),
                                workspace=ws.data_ptr(), stream=stream.cuda_stream)
        rc = _lib.lib.la3d_components_bits(C.byref(a))
        assert rc == 0, _lib.lib.la3d_last_error()

    side = torch.cuda.Stream()
    gr = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        run(side)                                                # (warm-up)
        side.synchronize()
        with torch.cuda.graph(gr, stream=side):
            run(torch.cuda.current_stream())
    for tag, masks in (("g1", first), ("g2", second)):
        src.bits.copy_(planes_of(la, masks, False).bits)         # changed planes in the captured buffers
        out.fill_(SENTINEL)
        stats.fill_(-7)
        tab.fill_(-7)
        ws.fill_(-1)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        check((la.MaskBits(out, H, W, W), stats, tab), src, *expect(labelled, [f"{tag}_{i}" for i in range(B)], masks, 8, 3, False, rows), tag)
