"""GPU tests of the annotation bit-plane packers (include/la3d.h "annotations as bit planes"; ``pack_rle_bits``, ``pack_poly_bits``,
``pack_rle_bits_frames``, ``pack_poly_bits_frames``): the planes against the CPU oracle, exactly, on the frame sizes that hit every
copy and decode form; the on-device refusals of the frames form; and the consumers - the fit and the instance point clouds - against
the routes a caller had before."""
import ctypes as C

import numpy as np
import pytest

from oracle import la3d_oracle as O

from . import annotation_bits_cases as AC
from . import frames_bits_cases as FC
from . import instance_points_cases as IC
from .conftest import SCHED

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
KINDS = ("rle", "poly")


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


def pack_uniform(la, kind, ann, H, W, **kw):
    if kind == "rle":
        return la.pack_rle_bits(AC.rle_objects(ann, H, W), **kw)
    return la.pack_poly_bits(la.pack_polygons(ann, H, W), **kw)


def pack_frames_form(la, kind, pf, ann, sizes, img, **kw):
    if kind == "rle":
        return la.pack_rle_bits_frames(pf, [{"size": list(sizes[p]), "counts": list(c)} for c, p in zip(ann, img)], img, **kw)
    return la.pack_poly_bits_frames(pf, la.pack_polygons(ann, 1, 1), img, **kw)


def check_uniform(mb, masks, H, W, W_out, area, tag):
    assert (mb.H, mb.W, mb.frame_width) == (H, W_out, W), tag
    got = u32(mb.bits)
    nwords = (H * W_out + 31) // 32
    assert got.shape[0] == len(masks) and got.shape[1] >= nwords
    for b, m in enumerate(masks):
        want = AC.words(m, W_out)
        np.testing.assert_array_equal(got[b, :nwords], want, err_msg=f"{tag}[{b}]")
        assert int(np_(area)[b]) == AC.popcount(want) == int(m.sum()), f"{tag}[{b}] area"


# ------------------------------------------------------------------------------------------
# 1. planes, one frame size per call
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W,pad", AC.UNIFORM, ids=[f"{h}x{w}{'p' if p else ''}" for h, w, p in AC.UNIFORM])
def test_planes_equal_the_oracle(la, kind, H, W, pad):
    import torch

    ann, masks = AC.expected(kind, H, W)
    area = torch.full((len(ann),), -1, dtype=torch.int32, device="cuda")
    mb = pack_uniform(la, kind, ann, H, W, frame_pad=pad, area=area)
    check_uniform(mb, masks, H, W, AC.padded(W) if pad else W, area, f"{kind} {H}x{W} pad={pad}")
    if kind == "rle":   # every list does what its name says
        n = H * W
        assert masks[0].sum() == 0 and masks[1].all() and masks[2].reshape(-1, order="F")[:5].all()
        assert masks[6].reshape(-1, order="F")[n - 3:].all() and masks[8].reshape(-1, order="F")[1:min(n, AC.NT_DEC + 131):2].all()
    else:
        assert masks[0].any() and masks[1].any() and masks[4].any() and masks[5].any() and not masks[6].any()


@pytest.mark.parametrize("kind", KINDS)
def test_planes_of_a_640x480_batch(la, kind):
    import torch

    H, W = AC.BIG
    ann, masks = AC.expected(kind, H, W)
    pick = (3, 7, 8) if kind == "rle" else (1, 3, 4)
    area = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    mb = pack_uniform(la, kind, [ann[i] for i in pick], H, W, area=area)
    check_uniform(mb, [masks[i] for i in pick], H, W, W, area, f"{kind} 480x640")
    # the consumers of planes read them back as the decoders' masks
    np.testing.assert_array_equal(np_(la.unpack_mask_bits(mb)), np.stack([masks[i] for i in pick]))


@pytest.mark.parametrize("kind", KINDS)
def test_out_reuse_and_a_stride_larger_than_a_plane(la, kind):
    """``out=`` is filled in place; the words between two planes keep their fill - with a 16-byte aligned base and stride (16-byte
    stores) and with a base 4 bytes off (word by word)"""
    import torch

    H, W = 75, 64
    ann, masks = AC.expected(kind, H, W)
    B, nwords = len(ann), H * W // 32
    for shift, gap in ((0, 6), (1, 5)):
        whole = torch.full((B, shift + nwords + gap), SENTINEL, dtype=torch.int32, device="cuda")
        out = whole[:, shift:]
        area = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        for _ in range(2):   # the second call overwrites the first
            mb = pack_uniform(la, kind, ann, H, W, out=out, area=area)
        assert mb.bits.data_ptr() == out.data_ptr()
        check_uniform(mb, masks, H, W, W, area, f"{kind} out shift={shift}")
        got = u32(whole)
        assert (got[:, :shift] == SENTINEL).all() and (got[:, shift + nwords:] == SENTINEL).all(), "a word outside a plane was written"


@pytest.mark.parametrize("kind", KINDS)
def test_one_pack_call_captured_into_a_graph(la, kind):
    import torch

    H, W = 33, 47
    ann, masks = AC.expected(kind, H, W)
    B, W_out = len(ann), AC.padded(W)
    dev = torch.device("cuda", 0)
    if kind == "rle":
        c, o, _, _ = la.pack_rle(AC.rle_objects(ann, H, W))
        src = (torch.as_tensor(c, device=dev), torch.as_tensor(o, device=dev), H, W)
        call = la.pack_rle_bits
    else:
        xy, ro, ir, _, _ = la.pack_polygons(ann, H, W)
        src = (torch.as_tensor(xy, device=dev), torch.as_tensor(ro, device=dev), torch.as_tensor(ir, device=dev), H, W)
        call = la.pack_poly_bits
    out = torch.zeros((B, (H * W_out + 31) // 32), dtype=torch.int32, device=dev)
    area = torch.zeros(B, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        call(src, out=out, area=area, stream=side)                      # (warm-up: the kernel's LDS attribute is set)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            mb = call(src, out=out, area=area, stream=torch.cuda.current_stream())
    for replay in range(2):
        out.fill_(SENTINEL)
        area.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check_uniform(mb, masks, H, W, W_out, area, f"{kind} replay {replay}")


# ------------------------------------------------------------------------------------------
# 2. planes of images of different sizes in one call
# ------------------------------------------------------------------------------------------
def mixed_batch(kind):
    """every annotation of every MIXED size, in scrambled image order -> (annotations, masks, image index)"""
    ann, masks, img = [], [], []
    for p, (h, w) in enumerate(AC.MIXED):
        a, m = AC.expected(kind, h, w)
        keep = range(len(a)) if (h, w) != AC.BIG else ((3, 7, 8) if kind == "rle" else (1, 3, 4))
        for i in keep:
            ann.append(a[i]); masks.append(m[i]); img.append(p)
    perm = np.random.RandomState(11).permutation(len(ann))
    return [ann[i] for i in perm], [masks[i] for i in perm], np.asarray(img, np.int32)[perm]


def depth_frames(la, sizes, seed=3):
    rs = np.random.RandomState(seed)
    return la.pack_frames([rs.uniform(0.5, 10, s).astype(np.float32) for s in sizes])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("index", ["host", "device"])
def test_frames_planes_equal_the_oracle(la, kind, index):
    import torch

    ann, masks, img = mixed_batch(kind)
    pf = depth_frames(la, AC.MIXED)
    ii = img if index == "host" else torch.as_tensor(img, device="cuda")
    fb = pack_frames_form(la, kind, pf, ann, AC.MIXED, ii)
    offs, bits, area = np_(fb.offsets), u32(fb.bits), np_(fb.area)
    np.testing.assert_array_equal(np_(fb.image_index), img)
    if index == "host":
        np.testing.assert_array_equal(offs, la.frame_bits_offsets(pf.table_host, img)[0])
    else:
        stride = (pf.H * pf.W // 32 + 3) // 4 * 4
        np.testing.assert_array_equal(offs, np.arange(len(img)) * stride)
    for b, (m, p) in enumerate(zip(masks, img)):
        want = AC.words(m, AC.padded(AC.MIXED[p][1]))
        np.testing.assert_array_equal(bits[offs[b]:offs[b] + len(want)], want, err_msg=f"{kind} row {b} image {p}")
        assert area[b] == AC.popcount(want) == m.sum(), (b, p)


@pytest.mark.parametrize("kind", KINDS)
def test_frames_refusals_write_nothing(la, kind):
    """a bad image index, a frame row with pitch 33 and a plane offset of 2 are refused on the device: area 0, the words of their
    planes keep the fill of a pre-filled ``out`` - as does everything outside the planes -, and the neighbours stay exact"""
    import torch

    from labelany3d_amd import _lib
    from labelany3d_amd import frames as frames_module

    sizes = AC.MIXED[:5]
    ann, masks, img = [], [], []
    for p, (h, w) in enumerate(sizes):
        a, m = AC.expected(kind, h, w)
        for i in (2, 3, 7) if kind == "rle" else (0, 2, 3):
            ann.append(a[i]); masks.append(m[i]); img.append(p)
    img = np.asarray(img, np.int32)
    B = len(img)
    pf = depth_frames(la, sizes)
    BROKEN = 2
    table = pf.table.clone()
    table[BROKEN, 3] = 33                                             # W (the pitch) of image 2: no multiple of 32
    offs_h, total = la.frame_bits_offsets(pf.table_host, img)
    outside, two = int(np.flatnonzero(img == 0)[1]), int(np.flatnonzero(img == 4)[0])
    ii_bad, offs_bad = img.copy(), offs_h.copy()
    ii_bad[outside], offs_bad[two] = len(sizes), 2
    refused = img == BROKEN
    refused[[outside, two]] = True
    assert refused.sum() == 5 and all(masks[b].any() for b in np.flatnonzero(refused))
    MARGIN = 1024
    whole = torch.full((MARGIN + total + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
    bits = whole[MARGIN:]
    area = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ii_t, offs_t = torch.as_tensor(ii_bad, device="cuda"), torch.as_tensor(offs_bad, device="cuda")
    p_ = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    tail = (p_(table), len(sizes), pf.H, pf.W, p_(ii_t), B, p_(bits), p_(offs_t), p_(area), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if kind == "rle":
        c, o, _ = frames_module.pack_rle_frames([{"size": list(sizes[p]), "counts": list(a)} for a, p in zip(ann, img)])
        src = [torch.as_tensor(c, device="cuda"), torch.as_tensor(o, device="cuda")]
        rc = _lib.lib.la3d_pack_rle_bits_frames(*[p_(t) for t in src], *tail)
    else:
        xy, ro, ir, _, _ = la.pack_polygons(ann, 1, 1)
        src = [torch.as_tensor(xy, device="cuda"), torch.as_tensor(ro, device="cuda"), torch.as_tensor(ir, device="cuda")]
        rc = _lib.lib.la3d_pack_poly_bits_frames(*[p_(t) for t in src], *tail)
    assert rc == 0, _lib.lib.la3d_last_error()
    torch.cuda.synchronize()
    want = np.full(whole.numel(), SENTINEL, np.uint32)
    want_area = np.zeros(B, np.int64)
    for b in np.flatnonzero(~refused):
        w = AC.words(masks[b], AC.padded(sizes[img[b]][1]))
        want[MARGIN + offs_h[b]:MARGIN + offs_h[b] + len(w)] = w
        want_area[b] = masks[b].sum()
    np.testing.assert_array_equal(u32(whole), want, err_msg="a refused row was written (or a conforming one missed)")
    np.testing.assert_array_equal(np_(area), want_area)


# ------------------------------------------------------------------------------------------
# 3. consumers: the fit
# ------------------------------------------------------------------------------------------
def same_records(got, other, tag):
    """status equal; records to the 1e-12 tests/test_gpu_frames_bits.py holds bit planes to against run lengths"""
    np.testing.assert_array_equal(np_(got[1]), np_(other[1]), err_msg=f"{tag} status")
    np.testing.assert_allclose(np.nan_to_num(np_(got[0]), nan=-7.0), np.nan_to_num(np_(other[0]), nan=-7.0), rtol=1e-12, atol=1e-12,
                               err_msg=f"{tag} records")


def on_instance_engine(fn, *a, **k):
    """the annotation entry pinned to the engine bit planes run on"""
    SCHED().engine = "instance"
    try:
        return fn(*a, **k)
    finally:
        SCHED().engine = None


def uniform_scene(kind, H, W):
    """-> (depth (B,H,W), K (B,3,3), annotations as the entries take them, masks)"""
    if kind == "rle":
        masks = IC.standard_masks(H, W)
        ann = [O.rle_encode(m) for m in masks]
    else:
        segs, masks = AC.expected("poly", H, W)
        masks = np.stack(masks)
        ann = segs
    B = len(masks)
    return IC.special_depth(B, H, W), IC.cameras(B, H, W), ann, masks


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", [(96, 224), (100, 214)])
def test_fit_on_packed_planes_equals_the_annotation_entry(la, kind, H, W):
    depth, K, ann, masks = uniform_scene(kind, H, W)
    if kind == "rle":
        got = la.fit_instances_bits(depth, la.pack_rle_bits(ann), K, height_rule="rows")
        ref = on_instance_engine(la.fit_instances_rle, depth, ann, K)
    else:
        polys = la.pack_polygons(ann, H, W)
        got = la.fit_instances_bits(depth, la.pack_poly_bits(polys), K, height_rule="span")
        ref = on_instance_engine(la.fit_instances_poly, depth, polys, K)
    same_records(got, ref, f"{kind} {H}x{W}")
    assert (np_(got[1]) == 0).sum() >= 3


@pytest.mark.parametrize("kind", KINDS)
def test_frames_fit_on_packed_planes_equals_the_annotation_entry(la, kind):
    case = FC.make_case(2)
    pf = la.pack_frames(case["depth"])
    img = case["img"]
    if kind == "rle":
        rles = [O.rle_encode(m) for m in case["masks"]]
        fb = la.pack_rle_bits_frames(pf, rles, img)
        ref = la.fit_instances_frames(pf, case["K"], rles=rles, image_index=img)
        rule = "rows"
    else:
        segs = [AC.polygons(*case["sizes"][p])[b % 6] for b, p in enumerate(img)]
        polys = la.pack_polygons(segs, 1, 1)
        fb = la.pack_poly_bits_frames(pf, polys, img)
        ref = la.fit_instances_frames(pf, case["K"], polys=polys, image_index=img)
        rule = "span"
    got = la.fit_instances_frames_bits(pf, fb, case["K"], height_rule=rule, area_hint=fb.area)
    same_records([got[k] for k in ("boxes", "status")], [ref[k] for k in ("boxes", "status")], f"frames {kind}")
    assert (np_(got["status"]) == 0).sum() >= 12


# ------------------------------------------------------------------------------------------
# 4. consumers: the instance point clouds
# ------------------------------------------------------------------------------------------
TOL = dict(rtol=1e-13, atol=1e-13)   # (the restatement's own bound, tests/test_gpu_instance_points.py)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", [(33, 47), (96, 224)])
def test_instance_points_on_packed_planes(la, kind, H, W):
    """bit for bit the clouds of the decoded boolean planes (NaN = NaN), and the NumPy restatement"""
    depth, K, ann, masks = uniform_scene(kind, H, W)
    if kind == "rle":
        mb, planes = la.pack_rle_bits(ann), la.rle_decode(ann)
    else:
        polys = la.pack_polygons(ann, H, W)
        mb, planes = la.pack_poly_bits(polys), la.poly_decode(polys)
    np.testing.assert_array_equal(np_(planes), masks)
    got = la.instance_points(depth, mb, K, pixels=True)
    old = la.instance_points(depth, planes, K, pixels=True)
    plain = la.instance_points(depth, la.MaskBits(*mb), K, pixels=True)     # the same planes without the packer's "checked" mark
    assert getattr(mb, "_stride", None) is not None and getattr(la.MaskBits(*mb), "_stride", None) is None
    for name in ("points", "offsets", "counts", "pixels", "status"):
        np.testing.assert_array_equal(np_(getattr(got, name)), np_(getattr(old, name)), err_msg=f"{kind} {name}")
        np.testing.assert_array_equal(np_(getattr(got, name)), np_(getattr(plain, name)), err_msg=f"{kind} {name} (plain MaskBits)")
    want = IC.cloud_rule(depth, masks, K)
    np.testing.assert_array_equal(np_(got.offsets), want[2])
    np.testing.assert_array_equal(np_(got.counts), want[3])
    np.testing.assert_array_equal(np_(got.pixels), want[1])
    np.testing.assert_allclose(np_(got.points), want[0], **TOL)
    assert want[3].sum() > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_instance_points_frames_on_packed_planes(la, kind, dtype):
    """per image the NumPy restatement on the image's own (up-converted) depth plane"""
    ann, masks, img = mixed_batch(kind)
    rs = np.random.RandomState(5)
    sizes = AC.MIXED
    K = IC.cameras(len(sizes), 64, 64)
    if dtype == "f32":
        planes = [IC.special_depth(1, h, w, seed=p)[0] for p, (h, w) in enumerate(sizes)]
        pf, up = la.pack_frames(planes), planes
    else:
        scale = np.float32(0.001)
        stored = [rs.randint(0, 9000, s).astype(np.uint16) for s in sizes]
        up = [np.where(s == 0, np.float32(np.nan), s.astype(np.float32) * scale).astype(np.float32) for s in stored]
        pf = la.pack_frames(stored, dtype="u16", scale=0.001, zero_is_hole=True)
    fb = pack_frames_form(la, kind, pf, ann, sizes, img)
    ip = la.instance_points_frames(pf, fb, K, pixels=True)
    pts, off, pix = np_(ip.points), np_(ip.offsets), np_(ip.pixels)
    np.testing.assert_array_equal(np_(ip.status), 0)
    np.testing.assert_array_equal(np_(ip.counts), [m.sum() for m in masks])
    for b, (m, p) in enumerate(zip(masks, img)):
        want = IC.cloud_rule(up[p], m[None], K[p])
        np.testing.assert_allclose(pts[off[b]:off[b + 1]], want[0], err_msg=f"row {b} image {p}", **TOL)
        np.testing.assert_array_equal(pix[off[b]:off[b + 1]], want[1], err_msg=f"row {b} image {p}")
