"""GPU tests of the depth gate on bit planes (include/la3d.h "depth gate on bit planes"; ``gate_depth_bits``, ``depth_gate_stats``):
planes and counts exact and levels equal against the NumPy restatement of the rule (tests/depth_gate_cases.py) on every generator
case - frame shapes, mask contents, garbage in the bits that are not image, both selection paths, invalid pixels, the scalars -; the
depth layouts, plane strides and batch sizes; in place, statistics only, two runs; one captured call; the fit downstream; the case the
feature exists for."""
import numpy as np
import pytest

from . import depth_gate_cases as DG

pytestmark = pytest.mark.gpu

SENTINEL = DG.SENTINEL


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


def dev(a, dtype=None):
    import torch

    t = torch.as_tensor(np.array(a), device="cuda")              # (a copy: the shared cases are read-only)
    return t if dtype is None else t.to(dtype)


def planes_of(la, masks, W_stored, garbage=None):
    """bool (B, H, W) -> MaskBits stored W_stored wide, made on the host (``garbage``: words OR-ed into every plane)"""
    words = DG.pack(masks, W_stored)
    if garbage is not None:
        words = words | garbage[None]
    B, H, W = np.shape(masks)
    return la.MaskBits(dev(words.view(np.int32)), H, W_stored, W)


def check(res, want, src, tag):
    """res: (MaskBits, DepthGateStats) of the call; want: (keep, counts, levels) of the restatement; src: the input MaskBits"""
    mb, stats = res
    keep, counts, levels = want
    assert (mb.H, mb.W, mb.frame_width) == (src.H, src.W, src.frame_width), tag
    nwords = (mb.H * mb.W + 31) // 32
    got = u32(mb.bits)[:, :nwords]
    want_words = DG.pack(keep, mb.W)
    bad = np.flatnonzero((got != want_words).any(1))
    assert bad.size == 0, (tag, "planes", bad[:8].tolist())
    got_counts, got_levels = np_(stats.counts), np_(stats.levels)
    assert got_counts.dtype == np.int32 and got_levels.dtype == np.float32 and got_counts.shape == got_levels.shape == (len(keep), 3), tag
    assert np.array_equal(got_counts, counts), (tag, "counts", got_counts[(got_counts != counts).any(1)][:4], counts[(got_counts != counts).any(1)][:4])
    assert np.array_equal(got_levels, levels, equal_nan=True), (tag, "levels", got_levels[:4], levels[:4])


@pytest.mark.parametrize("H,W,pad", DG.FRAMES)
def test_every_case_of_a_frame_under_every_scalar_set(la, H, W, pad):
    """frame shapes x mask contents x depth contents (invalid pixels among them) x near / far / k / min_band, clean planes and planes with
    garbage in the bits that are not image: the output has zeros there and the results are the same"""
    names, depths, masks = DG.planes(H, W)
    Ws = DG.stored_width(W, pad)
    gap = DG.not_image(H, W, Ws)
    rs = np.random.RandomState(H * W)
    noise = rs.randint(0, 1 << 32, gap.shape, dtype=np.uint64).astype(np.uint32) & gap
    d = dev(DG.pad_depth(depths, Ws, fill=2.5))             # (a plausible depth under the pad columns: a gate that read them would show)
    clean, dirty = planes_of(la, masks, Ws), planes_of(la, masks, Ws, noise)
    for i, kw in enumerate(DG.PARAMS):
        want = DG.expected((H, W), i)
        check(la.gate_depth_bits(d, clean, return_stats=True, **kw), want, clean, (H, W, kw, "clean"))
        if gap.any():
            res = la.gate_depth_bits(d, dirty, return_stats=True, **kw)
            check(res, want, dirty, (H, W, kw, "garbage"))
            assert not (u32(res[0].bits) & gap[None]).any()
    if pad:                                                 # depth rows as wide as the image are padded by the call
        check(la.gate_depth_bits(dev(depths), clean, return_stats=True), DG.expected((H, W), 0), clean, (H, W, "frame-wide depth"))


def test_both_selection_paths_at_96x96(la):
    """9216 pixels, beyond the 6144 keys the LDS buffer holds: smooth depth (the sample brackets the median), constant depth (all ties),
    two levels at 50 / 50 and 49 / 51, shared mantissas, negative and mixed signs, invalid pixels, and counts on both sides of 6144"""
    names, depths, masks = DG.big_planes()
    H, W = DG.BIG
    src = planes_of(la, masks, W)
    d = dev(depths)
    for i, kw in enumerate(DG.PARAMS):
        check(la.gate_depth_bits(d, src, return_stats=True, **kw), DG.expected("big", i), src, ("big", kw))


def test_depth_layouts_strides_and_batch_sizes(la):
    import torch

    H, W, pad = DG.FRAMES[0]
    names, depths, masks = DG.planes(H, W)
    nwords = (H * W + 31) // 32
    # one shared plane, as (H, W) and as (1, H, W)
    shared = depths[names.index("invalid/full")]
    src = planes_of(la, masks, W)
    want = DG.gate_batch([shared] * len(masks), masks)
    check(la.gate_depth_bits(dev(shared), src, return_stats=True), want, src, "shared (H, W)")
    check(la.gate_depth_bits(dev(shared[None]), src, return_stats=True), want, src, "shared (1, H, W)")
    # (P = 2, H, W) with image_index over B = 5, on the host and on the device
    two = np.stack([depths[names.index("smooth/full")], depths[names.index("mixed/full")]])
    index = np.array([1, 0, 0, 1, 1], np.int32)
    m5 = masks[[names.index(f"smooth/{n}") for n in ("half", "odd", "full", "even", "two")]]
    src5 = planes_of(la, m5, W)
    want5 = DG.gate_batch(two[index], m5, k=1.0, min_band=0.05)
    for ii in (index, dev(index)):
        check(la.gate_depth_bits(dev(two), src5, k=1.0, min_band=0.05, image_index=ii, return_stats=True), want5, src5, "image_index")
    with pytest.raises(ValueError, match="image_index"):
        la.gate_depth_bits(dev(two), src5, image_index=np.array([0, 1, 2, 0, 0], np.int32))
    with pytest.raises(ValueError, match="image_index"):
        la.gate_depth_bits(dev(two), src5)
    # private (B, H, W) planes; a non-dense bits stride, once a multiple of four words (16-byte loads with three words behind them);
    # an out with a larger stride whose words beyond each plane stay untouched
    d = dev(depths)
    want = DG.expected((H, W), 0)
    assert nwords == 15
    for stride in (16, 17):
        wide = torch.full((len(masks), stride), SENTINEL, dtype=torch.int32, device="cuda")
        wide[:, :nwords] = src.bits
        view = la.MaskBits(wide[:, :nwords], H, W, W)
        out = torch.full((len(masks), nwords + 9), SENTINEL, dtype=torch.int32, device="cuda")
        mb, stats = la.gate_depth_bits(d, view, out=out, return_stats=True)
        assert mb.bits is out and (u32(out)[:, nwords:] == SENTINEL).all() and (u32(wide)[:, nwords:] == SENTINEL).all(), stride
        check((mb, stats), want, view, ("stride", stride))
    # B = 0, 1, 70
    empty = la.MaskBits(torch.zeros((0, nwords), dtype=torch.int32, device="cuda"), H, W, W)
    mb, stats = la.gate_depth_bits(dev(shared), empty, return_stats=True)
    assert tuple(mb.bits.shape) == (0, nwords) and tuple(stats.counts.shape) == tuple(stats.levels.shape) == (0, 3)
    assert tuple(la.depth_gate_stats(torch.zeros((0, H, W), device="cuda"), empty).counts.shape) == (0, 3)
    one = planes_of(la, masks[:1], W)
    check(la.gate_depth_bits(d[:1], one, return_stats=True), tuple(w[:1] for w in want), one, "B = 1")
    pick = np.arange(70) % len(masks)
    many = planes_of(la, masks[pick], W)
    check(la.gate_depth_bits(dev(depths[pick]), many, return_stats=True), tuple(w[pick] for w in want), many, "B = 70")


def test_in_place_statistics_only_and_two_runs(la):
    H, W, pad = DG.FRAMES[1]
    names, depths, masks = DG.planes(H, W)
    Ws = DG.stored_width(W, pad)
    d = dev(DG.pad_depth(depths, Ws))
    src = planes_of(la, masks, Ws, DG.not_image(H, W, Ws))
    kw = DG.PARAMS[2]
    want = DG.expected((H, W), 2)
    first = la.gate_depth_bits(d, src, return_stats=True, **kw)
    check(first, want, src, "out of place")
    second = la.gate_depth_bits(d, src, return_stats=True, **kw)
    assert second[0].bits.data_ptr() != first[0].bits.data_ptr()
    for a, b in ((first[0].bits, second[0].bits), (first[1].counts, second[1].counts), (first[1].levels, second[1].levels)):
        assert np.array_equal(u32(a), u32(b))               # two runs: bit-identical (levels compared as words)
    only = la.depth_gate_stats(d, src, **kw)                # no plane written, the same statistics
    assert isinstance(only, la.DepthGateStats)
    assert np.array_equal(np_(only.counts), want[1]) and np.array_equal(np_(only.levels), want[2], equal_nan=True)
    alone = la.gate_depth_bits(d, src, **kw)                # without return_stats: the planes alone
    assert isinstance(alone, la.MaskBits) and np.array_equal(u32(alone.bits), u32(first[0].bits))
    work = la.MaskBits(src.bits.clone(), src.H, src.W, src.frame_width)
    mb, stats = la.gate_depth_bits(d, work, out=work.bits, return_stats=True, **kw)
    assert mb.bits is work.bits
    check((mb, stats), want, src, "in place")
    with pytest.raises(la.La3dError, match="overlap"):      # any other overlap is refused
        la.gate_depth_bits(d[:-1], la.MaskBits(work.bits[:-1], src.H, src.W, src.frame_width), out=work.bits[1:], **kw)


def test_one_captured_call_replayed_on_changed_inputs(la):
    import torch

    H, W, pad = DG.FRAMES[0]
    names, depths, masks = DG.planes(H, W)
    nwords = (H * W + 31) // 32
    B = len(masks)
    src = la.MaskBits(torch.zeros((B, nwords), dtype=torch.int32, device="cuda"), H, W, W)
    d = torch.zeros((B, H, W), dtype=torch.float32, device="cuda")
    out = torch.zeros((B, nwords), dtype=torch.int32, device="cuda")
    kw = dict(k=1.0, min_band=0.05)
    side = torch.cuda.Stream()
    gr = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        la.gate_depth_bits(d, src, out=out, return_stats=True, **kw)     # (warm-up)
        side.synchronize()
        with torch.cuda.graph(gr, stream=side):
            mb, stats = la.gate_depth_bits(d, src, out=out, return_stats=True, **kw)
    order = np.arange(B)[::-1].copy()
    for tag, dd, mm in (("g1", depths, masks), ("g2", depths[order], masks[order])):
        src.bits.copy_(planes_of(la, mm, W).bits)           # changed planes and depths in the captured buffers
        d.copy_(dev(dd))
        out.fill_(SENTINEL)
        stats.counts.fill_(-7)
        stats.levels.fill_(-7.0)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        check((mb, stats), DG.gate_batch(dd, mm, **kw), src, tag)


K = np.array([[120.0, 0.0, 32.0], [0.0, 120.0, 24.0], [0.0, 0.0, 1.0]])


def test_the_fit_downstream_takes_the_gated_planes(la):
    """fit_instances_bits on the gated planes = fit_instances_bits on pack_mask_bits(keep) of the restatement: records and statuses"""
    H, W, pad = DG.FRAMES[1]
    names, depths, masks = DG.planes(H, W)
    Ws = DG.stored_width(W, pad)
    d = dev(DG.pad_depth(depths, Ws))
    src = planes_of(la, masks, Ws)
    gated = la.gate_depth_bits(d, src)
    keep = DG.expected((H, W), 0)[0]
    theirs = la.pack_mask_bits(dev(keep.astype(np.uint8)), frame_pad=True)
    assert (theirs.H, theirs.W, theirs.frame_width) == (gated.H, gated.W, gated.frame_width)
    got = la.fit_instances_bits(d, gated, K)
    want = la.fit_instances_bits(d, theirs, K)
    assert np.array_equal(np_(got[1]), np_(want[1]))
    assert np.array_equal(np_(got[0]), np_(want[0]), equal_nan=True) and np.array_equal(np_(got[2]), np_(want[2]), equal_nan=True)
    assert (np_(got[1]) == 0).sum() >= 5, np_(got[1])       # (the comparison is not one of refused instances)


def test_the_case_the_feature_exists_for(la):
    """a 48 x 64 instance at 2 m +- 5 cm whose mask bleeds four columns onto the wall at 7.5 m and holds one 10000.0 pixel: ungated the
    fitted box is kilometres deep, gated with the defaults it is the object's"""
    depth, mask = DG.scene()
    d = dev(depth)
    src = la.pack_mask_bits(dev(mask[None].astype(np.uint8)))

    def depth_extent(bits):
        boxes, status, _ = la.fit_instances_bits(d, bits, K)
        assert np_(status).tolist() == [0]
        z = np_(la.unpack_boxes(boxes)["bbox3D_cam"])[0, :, 2]
        return float(z.max() - z.min())

    assert depth_extent(src) > 1000
    gated, stats = la.gate_depth_bits(d, src, return_stats=True)
    check((gated, stats), DG.gate_batch([depth], [mask]), src, "scene")
    assert np_(stats.counts).tolist() == [[1280, 1280, 1151]]
    assert depth_extent(gated) < 0.5
