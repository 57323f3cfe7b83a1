"""GPU tests of the label-map mask source (include/la3d.h "masks as label maps"): ``pack_label_bits`` bit for bit against
``np.packbits(labels[image] == id)``, ``fit_instances_labels`` against the oracle and against ``fit_instances_bits`` on planes packed
on the host with ``np.packbits`` (never with the code under test), ``label_instances`` against ``np.unique``.  The comparison rules
are the suite's own (tests/test_gpu_bits.py): ``check_oracle``, and between two entries of one engine ``same_engine`` - status and
``aux[:, 1:3]`` equal, records to rtol = atol = 1e-12.  On every input here the restatement ``labels == id`` is exact: no case is
skipped or filtered."""
import numpy as np
import pytest

from oracle import la3d_oracle as O

from .test_gpu_bits import K224, K640, check_oracle, host_bits, np_, packbits, padded, same_engine, words

pytestmark = pytest.mark.gpu

K96 = np.array([[90.0, 0, 48], [0, 90.0, 32], [0, 0, 1]])
DTYPES = ("u8", "u16", "i32", "rgb8")
# ids every map of a dtype holds somewhere: the ends of the dtype's range
ENDS = {"u8": [0, 255], "u16": [0, 255, 256, 65535], "i32": [0, -5, -2**31, 2**31 - 1, 65536], "rgb8": [0, 255, 256, 65536, 2**24 - 1]}
# ids no map of the dtype can hold: all-zero planes, not errors
OUTSIDE = {"u8": [300, -1, 256], "u16": [65536, -1, 70000], "i32": [], "rgb8": [2**24, -1, 2**31 - 1]}
RANGE = {"u8": (0, 256), "u16": (0, 65536), "i32": (-2**31, 2**31), "rgb8": (0, 2**24)}


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def palette(rs, dtype, n):
    """n distinct ids of the dtype, its ends among them"""
    lo, hi = RANGE[dtype]
    ids = list(ENDS[dtype])
    while len(ids) < n:
        v = int(rs.randint(lo, hi, dtype=np.int64))
        if v not in ids:
            ids.append(v)
    return np.asarray(ids[:n], np.int64)


def voronoi(rs, H, W, n):
    """(H,W) cell index in [0, n): nearest of n random seeds under a random anisotropic metric"""
    vv, uu = np.mgrid[0:H, 0:W]
    sy, sx, a = rs.uniform(0, H, n), rs.uniform(0, W, n), rs.uniform(0.5, 2.0, n)
    return np.argmin(a[:, None, None] * (vv[None] - sy[:, None, None]) ** 2 + (uu[None] - sx[:, None, None]) ** 2 / a[:, None, None], axis=0)


def blocky(rs, H, W, n, bh=16, bw=24):
    """(H,W) cell index in [0, n): blocks of bh x bw pixels, each of a random cell"""
    g = rs.randint(0, n, ((H + bh - 1) // bh, (W + bw - 1) // bw))
    return np.kron(g, np.ones((bh, bw), np.int64))[:H, :W]


def encode(values, dtype):
    """true ids (int64, (..., H, W)) -> the array a caller holds"""
    if dtype == "u8":
        return values.astype(np.uint8)
    if dtype == "u16":
        return values.astype(np.uint16)
    if dtype == "i32":
        return values.astype(np.int32)
    return np.stack([values & 255, (values >> 8) & 255, (values >> 16) & 255], axis=-1).astype(np.uint8)


def resident(arr):
    """a NumPy label array on the device (uint16 goes up as its int16 bit pattern, which the packer reads as uint16)"""
    import torch

    return torch.as_tensor(arr.view(np.int16) if arr.dtype == np.uint16 else arr, device="cuda")


def expected(values, ids, W_out):
    """(words (B, nwords), areas (B,), masks (B,H,W), image_index) of the rows ``ids`` lists"""
    ii = np.repeat(np.arange(len(ids)), [len(x) for x in ids]).astype(np.int32)
    flat = np.concatenate([np.asarray(x, np.int64) for x in ids]) if len(ii) else np.zeros(0, np.int64)
    masks = values[ii] == flat[:, None, None] if len(ii) else np.zeros((0,) + values.shape[1:], bool)
    return packbits(masks, W_out), masks.reshape(len(ii), -1).sum(1), masks, ii


def check_pack(lb, want, areas, ii, H, W_out, W, tag):
    import torch

    assert (lb.bits.H, lb.bits.W, lb.bits.frame_width) == (H, W_out, W) and lb.bits.bits.dtype == torch.int32, tag
    np.testing.assert_array_equal(words(lb.bits.bits), want, err_msg=f"{tag} words")
    np.testing.assert_array_equal(np_(lb.area), areas, err_msg=f"{tag} area")
    np.testing.assert_array_equal(np_(lb.image_index), ii, err_msg=f"{tag} image_index")
    assert lb.area.dtype == torch.int32 and lb.image_index.dtype == torch.int32


# ------------------------------------------------------------------------------------------
# 1. the packer, bit for bit
# ------------------------------------------------------------------------------------------
# 64 x 96: vector form, less than one chunk of 256 words; 96 x 224: vector form, 2.6 chunks (chunk seams); 50 x 75 padded to 96
# columns: general form; 7 x 45 unpadded: general form with a ragged last word
SHAPES = [(64, 96, True), (96, 224, True), (50, 75, True), (7, 45, False)]


@pytest.mark.parametrize("H,W,pad", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_label_bits_equals_packbits(la, dtype, H, W, pad):
    import torch

    rs = np.random.RandomState(H * 31 + W + len(dtype))
    W_out = padded(W) if pad else W
    pal = palette(rs, dtype, 48)
    # image 0: a Voronoi map of 44 cells, 40 of them listed (past any unroll) + an absent id + a duplicated id + ids outside the
    # dtype; image 1: a blocky map, NO instances; image 2: a blocky map, 5 instances; image 3: uniformly random over 6 ids
    values = np.stack([pal[voronoi(rs, H, W, 44)], pal[blocky(rs, H, W, 9, 5, 7)], pal[blocky(rs, H, W, 9, 8, 11)],
                       pal[rs.randint(0, 6, (H, W))]])
    for k, e in enumerate(ENDS[dtype]):                           # the ends of the dtype's range are present in image 0 (and listed)
        values[0, k % H, (7 * k + 3) % W] = e
    absent = int(pal[47])
    assert not (values == absent).any()
    ids0 = [int(v) for v in pal[:40]] + [absent, int(pal[3]), int(pal[3])] + OUTSIDE[dtype]
    ids = [ids0, [], [int(v) for v in pal[[0, 1, 4, 8, 2]]], [int(v) for v in pal[:6]] + [int(pal[1])]]
    arr = encode(values, dtype)
    rgb = dtype == "rgb8"
    want, areas, masks, ii = expected(values, ids, W_out)
    assert len(ids0) > 40 and areas[40] == 0 and (areas[len(ids0) - len(OUTSIDE[dtype]):len(ids0)] == 0).all()
    assert (areas[:len(ENDS[dtype])] > 0).all() and list(pal[:len(ENDS[dtype])]) == ENDS[dtype]
    for name, src in (("numpy", arr), ("resident", resident(arr))):
        check_pack(la.pack_label_bits(src, ids, frame_pad=pad, rgb=rgb), want, areas, ii, H, W_out, W, f"{dtype} {W}x{H} {name}")
    # the flat form of the same rows, on the host and on the device
    flat = np.concatenate([np.asarray(x, np.int64) for x in ids]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.int32)
    check_pack(la.pack_label_bits(arr, (flat, off), frame_pad=pad, rgb=rgb), want, areas, ii, H, W_out, W, "flat host ids")
    check_pack(la.pack_label_bits(resident(arr), (torch.as_tensor(flat, device="cuda"), torch.as_tensor(off, device="cuda")), frame_pad=pad,
                                  rgb=rgb), want, areas, ii, H, W_out, W, "flat device ids")
    # P = 1, as (1,H,W) and as (H,W)
    w1, a1, _, i1 = expected(values[:1], ids[:1], W_out)
    check_pack(la.pack_label_bits(arr[:1], ids[:1], frame_pad=pad, rgb=rgb), w1, a1, i1, H, W_out, W, "P=1")
    check_pack(la.pack_label_bits(resident(arr[3]), ids[3:], frame_pad=pad, rgb=rgb), *expected(values[3:], ids[3:], W_out)[:2],
               np.zeros(len(ids[3]), np.int32), H, W_out, W, "(H,W)")
    # no instance at all
    lb = la.pack_label_bits(arr, [[], [], [], []], frame_pad=pad, rgb=rgb)
    assert tuple(lb.bits.bits.shape) == (0, want.shape[1]) and lb.area.numel() == 0 and lb.image_index.numel() == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_misaligned_base_and_wide_plane_stride_give_the_same_words(la, dtype):
    """a base one element past alignment and a plane stride above H*W: read where they lie, by the general form"""
    import torch

    H, W, P = 64, 96, 3
    rs = np.random.RandomState(11 + len(dtype))
    pal = palette(rs, dtype, 12)
    values = np.stack([pal[voronoi(rs, H, W, 12)] for _ in range(P)])
    ids = [[int(v) for v in pal[:7]], [int(pal[2])], [int(v) for v in pal[3:12]]]
    arr = encode(values, dtype)
    want, areas, _, ii = expected(values, ids, W)
    src = resident(arr)
    c = 3 if dtype == "rgb8" else 1
    for off, gap in ((1, 0), (0, 3), (1, 5), (0, 4)):
        flat = torch.zeros(off + P * (H * W + gap) * c + 16, dtype=src.dtype, device="cuda")
        shape, strides = ((P, H, W, 3), ((H * W + gap) * 3, W * 3, 3, 1)) if c == 3 else ((P, H, W), (H * W + gap, W, 1))
        view = torch.as_strided(flat, shape, strides, off)
        view.copy_(src)
        if off:
            assert view.data_ptr() % 16 != 0
        lb = la.pack_label_bits(view, ids, rgb=c == 3)
        check_pack(lb, want, areas, ii, H, W, W, f"{dtype} base +{off}, stride +{gap}")
    # every second plane of a larger stack: plane stride 2 H W
    big = torch.zeros((2 * P,) + tuple(src.shape[1:]), dtype=src.dtype, device="cuda")
    big[1::2] = src
    assert not big[1::2].is_contiguous()
    check_pack(la.pack_label_bits(big[1::2], ids, rgb=c == 3), want, areas, ii, H, W, W, f"{dtype} every second plane")


@pytest.mark.parametrize("H,W,pad", [(96, 224, True), (50, 75, True), (7, 45, False)])
def test_pack_into_a_wider_stride_leaves_the_gap_untouched(la, H, W, pad):
    import torch

    rs = np.random.RandomState(6)
    pal = palette(rs, "u16", 10)
    values = np.stack([pal[voronoi(rs, H, W, 10)] for _ in range(2)])
    ids = [[int(v) for v in pal[:5]], [int(v) for v in pal[4:8]]]
    W_out = padded(W) if pad else W
    want, areas, masks, ii = expected(values, ids, W_out)
    nw = want.shape[1]
    for extra in (1, 4, 7):
        out = torch.full((len(ii), nw + extra), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        lb = la.pack_label_bits(encode(values, "u16"), ids, frame_pad=pad, out=out)
        assert lb.bits.bits.data_ptr() == out.data_ptr()
        got = words(out)
        np.testing.assert_array_equal(got[:, :nw], want)
        assert (got[:, nw:] == 0x5A5A5A5A).all(), "the words between two planes were written"
        np.testing.assert_array_equal(np_(lb.area), areas)
        np.testing.assert_array_equal(np_(la.unpack_mask_bits(lb.bits)), masks)


# ------------------------------------------------------------------------------------------
# 2. the fit
# ------------------------------------------------------------------------------------------
_SCENES = {}


def scene(H, W):
    """P = 4 images, 3 to 9 instances each, depth U(0.5, 10) as tests/test_gpu_bits.py::rle_masks draws it; built once per frame"""
    if (H, W) not in _SCENES:
        rs = np.random.RandomState(H + W)
        P = 4
        depth = rs.uniform(0.5, 10, (P, H, W)).astype(np.float32)
        pal = palette(rs, "u16", 12)
        values = np.stack([pal[voronoi(rs, H, W, 11)] for _ in range(P)])
        # an unlisted background along the top, bottom and left borders: cells that reach the right border are what the fused filter
        # drops as truncated, the others it keeps
        values[:, :11] = values[:, -11:] = pal[11]
        values[:, :, :11] = pal[11]
        ids = [[int(v) for v in pal[rs.permutation(11)[:n]]] for n in (3, 9, 5, 7)]
        _, areas, masks, ii = expected(values, ids, W)
        ground = np.array([[0.02, -0.98, 0.1, 1.5]] * len(ii)) + 0.03 * rs.randn(len(ii), 4)
        _SCENES[(H, W)] = dict(depth=depth, values=values, labels=encode(values, "u16"), ids=ids, masks=masks, ii=ii, areas=areas,
                               ground=ground, K=K224 if W == 224 else K96)
    return _SCENES[(H, W)]


@pytest.mark.parametrize("H,W", [(96, 224), (64, 96)])
@pytest.mark.parametrize("variant", ["plain", "ground", "sample_idx", "image_size", "convex_hull"])
def test_fit_instances_labels(la, variant, H, W):
    s = scene(H, W)
    depth, masks, ii, K = s["depth"], s["masks"], s["ii"], s["K"]
    kw, okw = {}, {}
    if variant == "ground":
        kw = okw = dict(ground=s["ground"])
    elif variant == "sample_idx":
        assert (s["areas"] > 500).sum() >= 3 and (s["areas"] <= 500).any()
        sidx = la.draw_sample_idx(la.pack_label_bits(s["labels"], s["ids"]).area, np.random.RandomState(17))
        np.testing.assert_array_equal(sidx, la.draw_sample_idx(s["areas"], np.random.RandomState(17)))
        kw = okw = dict(sample_idx=sidx)
    elif variant == "image_size":
        kw = dict(image_size=(W, H))
    elif variant == "convex_hull":
        kw = dict(method="convex_hull")
    got = la.fit_instances_labels(depth, resident(s["labels"]), s["ids"], K, **kw)
    lb = got[-1]
    assert isinstance(lb, la.LabelBits) and len(got) == (5 if variant == "image_size" else 4)
    np.testing.assert_array_equal(np_(lb.area), s["areas"])
    np.testing.assert_array_equal(np_(lb.image_index), ii)
    np.testing.assert_array_equal(words(lb.bits.bits), packbits(masks, padded(W)))
    host = la.fit_instances_bits(depth, host_bits(masks), K, image_index=ii, **kw)
    same_engine(got, host, f"{variant} vs host-packed planes")
    if variant == "convex_hull":
        for a, b in zip(got[:3], host):                     # the same planes through the same engine: the very same numbers
            np.testing.assert_array_equal(np_(a), np_(b))
        st = np_(got[1])
        if (H, W) == (96, 224):
            assert 2 * (st == 0).sum() >= len(ii)
        else:   # 64 x 96: the column arrays of a full-mask hull call (8 W bytes) fill the whole bit image - every instance is refused
            assert (st[s["areas"] > 0] == 5).all() and np.isnan(np_(got[0])).all()
        return
    status = check_oracle(got, depth, masks, K, f"labels {variant} {W}x{H}", depth_index=ii, **okw)
    assert 2 * (status == 0).sum() >= len(ii)
    if variant == "image_size":
        boxes, b2 = np_(got[0]), np_(got[3])
        np.testing.assert_array_equal(b2, np_(host[3]))
        for n in range(len(ii)):
            if status[n] == 0:
                np.testing.assert_allclose(b2[n], np.ravel(O.project_boxes(boxes[n:n + 1], K, (W, H))), rtol=1e-9, atol=1e-9)
            else:
                assert np.isnan(b2[n]).all()


@pytest.mark.parametrize("H,W", [(96, 224), (64, 96)])
@pytest.mark.parametrize("rule", ["rows", "span"])
def test_fused_filter(la, rule, H, W):
    s = scene(H, W)
    depth, masks, ii, K = s["depth"], s["masks"], s["ii"], s["K"]
    bits = host_bits(masks)
    flt = {"boundary_threshold": 3, "scale_threshold": 300, "truncation_pixels": 40}
    got = la.fit_instances_labels(depth, s["labels"], s["ids"], K, filter=flt, height_rule=rule)
    assert len(got) == 5
    host = la.fit_instances_bits(depth, bits, K, image_index=ii, filter=flt, height_rule=rule)
    same_engine(got, host, f"filter {rule}")
    np.testing.assert_array_equal(np_(got[3]), np_(la.mask_stats_bits(bits, boundary_threshold=3)))
    np.testing.assert_array_equal(np_(got[3]), [O.mask_stats(m, 3) for m in masks])
    # filter=True: the reference's thresholds
    got = la.fit_instances_labels(depth, s["labels"], s["ids"], K, filter=True, height_rule=rule)
    same_engine(got, la.fit_instances_bits(depth, bits, K, image_index=ii, filter=True, height_rule=rule), f"filter=True {rule}")
    np.testing.assert_array_equal(np_(got[3]), np_(la.mask_stats_bits(bits)))
    keep = np.array([O.keep_instance(x, H, rule == "rows") for x in np_(got[3])])
    np.testing.assert_array_equal(np_(got[1]) == 6, ~keep)
    assert keep.any() and not keep.all()


def test_fit_from_float16_depth(la):
    """a ``Depth16`` gives the records the float32 call gives on the up-converted planes (the rule of tests/test_gpu_depth16.py)"""
    import torch

    s = scene(96, 224)
    stored = s["depth"].astype(np.float16)
    up = stored.astype(np.float32)
    got = la.fit_instances_labels(la.Depth16(torch.as_tensor(stored, device="cuda")), s["labels"], s["ids"], s["K"], ground=s["ground"])
    check_oracle(got, up, s["masks"], s["K"], "float16 depth", depth_index=s["ii"], ground=s["ground"])
    same_engine(got, la.fit_instances_labels(up, s["labels"], s["ids"], s["K"], ground=s["ground"]), "float16 vs float32 on the up-converted planes")


# ------------------------------------------------------------------------------------------
# 3. once at the benchmark's frame: 640 x 480, 8 images of 7 instances
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["u8", "rgb8"])
def test_640x480(la, dtype):
    H, W, P = 480, 640, 8
    rs = np.random.RandomState(640 + len(dtype))
    pal = palette(rs, dtype, 9)
    values = np.stack([pal[blocky(rs, H, W, 9, 96, 128)] for _ in range(P)])
    ids = [[int(v) for v in pal[rs.permutation(9)[:7]]] for _ in range(P)]
    depth = rs.uniform(0.5, 10, (P, H, W)).astype(np.float32)
    want, areas, masks, ii = expected(values, ids, W)
    got = la.fit_instances_labels(depth, resident(encode(values, dtype)), ids, K640, rgb=dtype == "rgb8")
    check_pack(got[-1], want, areas, ii, H, W, W, f"{dtype} 640x480")
    status = check_oracle(got, depth, masks, K640, f"{dtype} 640x480", depth_index=ii)
    assert (status == 0).sum() >= len(ii) - P


# ------------------------------------------------------------------------------------------
# 4. label_instances
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["u8", "rgb8"])
def test_label_instances(la, dtype):
    H, W, P = 96, 224, 3
    rs = np.random.RandomState(4 + len(dtype))
    pal = palette(rs, dtype, 14)
    values = np.stack([pal[voronoi(rs, H, W, 13)] for _ in range(P)])
    values[:, :3, :5] = pal[13]                                   # a small segment in every image: dropped by min_area
    arr = encode(values, dtype)
    rgb = dtype == "rgb8"
    small = int((values[0] == pal[13]).sum())
    for ignore, min_area in (((0,), 1), ((0, int(pal[2])), 1), ((), small + 1), ((int(pal[1]),), 200)):
        for src in (arr, resident(arr)):
            ids, areas = la.label_instances(src, ignore=ignore, min_area=min_area, rgb=rgb)
            assert len(ids) == len(areas) == P
            for p in range(P):
                u, c = np.unique(values[p], return_counts=True)
                keep = ~np.isin(u, list(ignore)) & (c >= min_area)
                np.testing.assert_array_equal(ids[p], u[keep], err_msg=f"ignore={ignore} min_area={min_area} image {p}")
                np.testing.assert_array_equal(areas[p], c[keep])
    # its output, fed to the fit: exactly those instances
    ids, areas = la.label_instances(resident(arr), ignore=(0,), min_area=200, rgb=rgb)
    depth = rs.uniform(0.5, 10, (P, H, W)).astype(np.float32)
    got = la.fit_instances_labels(depth, arr, ids, K224, rgb=rgb)
    want, a, masks, ii = expected(values, ids, W)
    np.testing.assert_array_equal(a, np.concatenate(areas))
    check_pack(got[-1], want, a, ii, H, W, W, "label_instances -> fit")
    assert len(ii) == sum(len(x) for x in ids) and tuple(got[0].shape) == (len(ii), 39)
    check_oracle(got, depth, masks, K224, "label_instances -> fit", depth_index=ii)


# ------------------------------------------------------------------------------------------
# 5. captured into a graph
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(96, 224), (50, 75)])
def test_pack_label_bits_captured_into_a_graph(la, H, W):
    """resident arguments and ``out=``: a linear chain on one stream - the clear of ``area`` included -, captured once, replayed on
    fresh labels"""
    import torch

    dev = torch.device("cuda", 0)
    P = 3
    rs = np.random.RandomState(50 + H)
    pal = palette(rs, "i32", 9)
    ids = [[int(v) for v in pal[:4]], [], [int(v) for v in pal[2:9]]]
    flat = torch.as_tensor(np.concatenate([np.asarray(x, np.int64) for x in ids]).astype(np.int32), device=dev)
    off = torch.as_tensor(np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.int32), device=dev)
    B, W_out = int(flat.numel()), padded(W)
    labels = torch.zeros((P, H, W), dtype=torch.int32, device=dev)
    out = torch.zeros((B, (H * W_out + 31) // 32), dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        la.pack_label_bits(labels, (flat, off), out=out, stream=side)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            lb = la.pack_label_bits(labels, (flat, off), out=out, stream=torch.cuda.current_stream())
    for seed in (1, 2):
        r2 = np.random.RandomState(seed)
        values = np.stack([pal[voronoi(r2, H, W, 9)] for _ in range(P)])
        labels.copy_(torch.as_tensor(encode(values, "i32"), device=dev))
        want, areas, _, ii = expected(values, ids, W_out)
        for replay in range(2):                               # twice on the same labels: the areas are cleared, not accumulated
            out.fill_(0x5A5A5A5A)
            g.replay()
            torch.cuda.synchronize()
            check_pack(lb, want, areas, ii, H, W_out, W, f"seed {seed} replay {replay}")
