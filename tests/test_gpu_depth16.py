"""GPU tests of the 16-bit depth source (include/la3d.h "16-bit depth planes"): ``Depth16`` through every fit entry that takes it,
``pack_depth16`` / ``unpack_depth16`` against the NumPy rules.  The results contract: a 16-bit call gives the records the float32
call gives on the up-converted planes.  Two comparison rules, both the suite's own:
  * against the oracle on the up-converted planes: ``assert_records`` with the call's ``aux[:, 3]`` as gap, status / n_valid / n_masked
    equal (``check_oracle`` of tests/test_gpu_bits.py; ``check_against_oracle`` of tests/test_gpu_hull_instances.py for hull records);
  * against the float32 entry pinned to the instance engine on the up-converted planes: the ``same_engine`` rule of
    tests/test_gpu_bits.py - status and ``aux[:, 1:3]`` equal, records to rtol = atol = 1e-12.  An inexact conversion (a contracted
    u * scale, a flushed subnormal, the wrong half of a packed pair) is 1e-8 relative or more.
The planes are quantised in tests/depth16_cases.py with NumPy, never with the packer under test; every instance of every case is
compared."""
import numpy as np
import pytest

from oracle import la3d_oracle as O

from . import depth16_cases as DC
from .conftest import SCHED
from .test_gpu_bits import check_oracle, host_bits, np_, same_engine
from .test_gpu_hull_instances import check_against_oracle as check_hull_against_oracle

pytestmark = pytest.mark.gpu

CASES = DC.fixed_cases()
VARIANTS = list(zip(DC.VARIANTS, DC.VARIANT_IDS))


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def dev16(la, stored, variant, frame_width=0):
    """the stored planes, uploaded, as a Depth16 (uint16 goes up as its int16 bit pattern)"""
    import torch

    _, scale, hole = variant
    if stored.dtype == np.float16:
        return la.Depth16(torch.as_tensor(stored, device="cuda"), 1.0, True, frame_width)
    return la.Depth16(torch.as_tensor(np.ascontiguousarray(stored).view(np.int16), device="cuda").view(torch.uint16), scale, hole, frame_width)


def fit(la, entry, depth, masks, K, segs=None, pinned=False, **kw):
    """one call of the entry a case names; ``pinned``: on the instance engine (the float32 side of the same_engine rule)"""
    H, W = masks.shape[1:]
    if pinned:
        SCHED().engine = "instance"
    try:
        if entry == "u8":
            return la.fit_instances(depth, masks, K, **kw)
        if entry == "rle":
            return la.fit_instances_rle(depth, [O.rle_encode(m) for m in masks], K, **kw)
        if entry == "poly":
            return la.fit_instances_poly(depth, la.pack_polygons(segs, H, W), K, **kw)
        return la.fit_instances_bits(depth, host_bits(masks), K, **kw)
    finally:
        SCHED().engine = None


def both_rules(la, got, up, case_kw, masks, K, tag, entry="u8", segs=None, method="pca", want=None):
    """the 16-bit records against the oracle on the up-converted planes and against the float32 entry on the instance engine"""
    kw = {k: v for k, v in case_kw.items() if v is not None}
    okw = dict(ground=kw.get("ground"), sample_idx=kw.get("sample_idx"), depth_index=kw.get("image_index"))
    if method == "convex_hull":
        check_hull_against_oracle(got[:3], up, masks, K, tag, **okw)
        status = np_(got[1])
    else:
        status = check_oracle(got, up, masks, K, tag, **okw)
    if want is not None:
        np.testing.assert_array_equal(status, want, err_msg=f"{tag}: expected statuses")
    ref = fit(la, entry, up, masks, K, segs=segs, pinned=True, method=method, **kw)
    same_engine(got, ref, tag + " vs float32 on the instance engine")
    return status


# ------------------------------------------------------------------------------------------
# 1. - 3. every walk, every mask source, special values: the fixed cases of tests/depth16_cases.py
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixed_cases(la, case, variant, vid):
    stored, up, want, sidx = DC.materialise(case, variant)
    kw = dict(ground=case["ground"], sample_idx=sidx, image_index=case["ii"])
    got = fit(la, case["entry"], dev16(la, stored, variant), case["masks"], case["K"], segs=case["segs"], method=case["method"],
              **{k: v for k, v in kw.items() if v is not None})
    both_rules(la, got, up, kw, case["masks"], case["K"], f"{case['name']} [{vid}]", case["entry"], case["segs"], case["method"], want)


@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
def test_fused_filter_both_height_rules_and_proj(la, variant, vid):
    """the fused filter on the annotation and bit sources (both height rules), proj with per-image K and planes shared through image_index"""
    rs = np.random.RandomState(21)
    B, Pn, H, W = 16, 3, 96, 224
    masks = np.zeros((B, H, W), bool)
    for i in range(B):
        h, w = rs.randint(8, H - 24), rs.randint(12, W - 24)
        r0, c0 = rs.randint(11, H - 11 - h + 1), rs.randint(11, W - 11 - w + 1)
        masks[i, r0:r0 + h, c0:c0 + w] = True
    masks[3] = False; masks[3, 40:44, 50:54] = True               # below min_area
    masks[5] = False; masks[5, 0:60, 0:40] = True                 # touches the border
    masks[7] = False; masks[7, 20:23, 40:60] = True; masks[7, 60:63, 40:60] = True   # six rows holding pixels, a span of 43
    masks[9] = False                                              # empty
    stored = DC.quantise(DC.smooth_depth(rs, Pn, H, W), variant[0], variant[1])
    up = DC.upconvert(stored, variant[1], variant[2])
    d16 = dev16(la, stored, variant)
    ii = (np.arange(B) % Pn).astype(np.int32)
    Ks = np.stack([DC.K224, DC.K224 * [[1.1], [0.9], [1]], DC.K224 * [[0.9], [1.2], [1]]])
    rles = [O.rle_encode(m) for m in masks]
    stats_want = np.array([O.mask_stats(m) for m in masks])
    for rule, from_rle in (("rows", True), ("span", False)):
        keep = np.array([O.keep_instance(s, H, from_rle) for s in stats_want])
        got = la.fit_instances_bits(d16, host_bits(masks), Ks, image_index=ii, filter=True, height_rule=rule, image_size=(W, H))
        ref = la.fit_instances_bits(up, host_bits(masks), Ks, image_index=ii, filter=True, height_rule=rule, image_size=(W, H))
        assert len(got) == 5
        np.testing.assert_array_equal(np_(got[3]), stats_want, err_msg=f"{rule}: statistics")
        np.testing.assert_array_equal(np_(got[1]) == 6, ~keep, err_msg=f"{rule}: kept set")
        same_engine(got, ref, f"bits filter {rule} [{vid}]")
        np.testing.assert_allclose(np.nan_to_num(np_(got[4]), nan=-7.0), np.nan_to_num(np_(ref[4]), nan=-7.0), rtol=1e-12, atol=1e-12)
        boxes, status, b2 = np_(got[0]), np_(got[1]), np_(got[4])
        for n in range(B):
            if status[n] == 0:
                np.testing.assert_allclose(b2[n], np.ravel(O.project_boxes(boxes[n:n + 1], Ks[ii[n]], (W, H))), rtol=1e-9, atol=1e-9)
            else:
                assert np.isnan(b2[n]).all()
        # the fitted ones against the oracle: the kept instances only were fitted
        ref39, st, _, nv = O.fit_instances(up, masks, Ks, depth_index=ii)
        from .test_gpu_parity import assert_records
        ok = keep & (st == 0)
        assert ok.sum() >= B // 2
        np.testing.assert_array_equal(status[keep], st[keep])
        assert_records(boxes[ok], ref39[ok], f"filter {rule}", gap=np_(got[2])[ok, 3])
    SCHED().engine = "instance"
    try:
        for entry_kw, what in ((dict(rles=rles), "rle"), (dict(polys=None), "poly")):
            if what == "poly":
                segs = DC.ellipse_segs(np.random.RandomState(3), B, H, W)
                entry_kw = dict(polys=la.pack_polygons(segs, H, W))
            got = la.fit_instances_ex(d16, Ks, image_index=ii, filter=True, image_size=(W, H), **entry_kw)
            ref = la.fit_instances_ex(up, Ks, image_index=ii, filter=True, image_size=(W, H), **entry_kw)
            same_engine((got["boxes"], got["status"], got["aux"]), (ref["boxes"], ref["status"], ref["aux"]), f"{what} filter [{vid}]")
            np.testing.assert_array_equal(np_(got["stats"]), np_(ref["stats"]))
            np.testing.assert_allclose(np.nan_to_num(np_(got["boxes2d"]), nan=-7.0), np.nan_to_num(np_(ref["boxes2d"]), nan=-7.0), rtol=1e-12, atol=1e-12)
            assert (np_(got["status"]) == 0).sum() >= B // 2
    finally:
        SCHED().engine = None


# ------------------------------------------------------------------------------------------
# 4. layouts
# ------------------------------------------------------------------------------------------
def strided16(la, stored, variant, gap, off, sentinel):
    """the planes H*W + gap elements apart, the base ``off`` elements into an allocation, everything between them = sentinel"""
    import torch

    Pn, H, W = stored.shape
    bits = torch.as_tensor(np.ascontiguousarray(stored).view(np.int16), device="cuda")
    s16 = int(np.array([sentinel], stored.dtype).view(np.int16)[0])
    flat = torch.full((off + Pn * (H * W + gap) + 8,), s16, dtype=torch.int16, device="cuda")
    view = torch.as_strided(flat, (Pn, H, W), (H * W + gap, W, 1), off)
    view.copy_(bits)
    tdt = torch.float16 if stored.dtype == np.float16 else torch.uint16
    return la.Depth16(torch.as_strided(flat.view(tdt), (Pn, H, W), (H * W + gap, W, 1), off), variant[1] if tdt == torch.uint16 else 1.0, variant[2])


@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
@pytest.mark.parametrize("H,W", [(96, 224), (61, 75)])
def test_plane_stride_base_offset_and_shared_plane(la, H, W, variant, vid):
    rs = np.random.RandomState(H + W)
    B = 8
    masks = DC.blob_masks(rs, B, H, W)
    ground = DC.ground_rows(rs, B)
    K = DC.K224.copy()
    K[0, 2], K[1, 2] = W / 2, H / 2
    stored = DC.quantise(DC.smooth_depth(rs, B, H, W), variant[0], variant[1])
    up = DC.upconvert(stored, variant[1], variant[2])
    sentinel = 60000.0 if variant[0] == "f16" else 65535           # (read as a depth, either wrecks the record)
    for g in (None, ground):
        kw = dict(ground=g)
        dense = la.fit_instances(dev16(la, stored, variant), masks, K, **{k: v for k, v in kw.items() if v is not None})
        both_rules(la, dense, up, kw, masks, K, f"dense {W}x{H} [{vid}]")
        for gap, off in ((8, 0), (64, 8)):                         # the vector form keeps its alignment: the same walk, the same records
            got = la.fit_instances(strided16(la, stored, variant, gap, off, sentinel), masks, K, **{k: v for k, v in kw.items() if v is not None})
            for a, b in zip(got, dense):
                np.testing.assert_array_equal(np_(a), np_(b), err_msg=f"stride +{gap}, base +{off}")
        for gap, off in ((3, 0), (0, 1), (6, 3)):                  # 2-byte aligned only: the general form
            d16 = strided16(la, stored, variant, gap, off, sentinel)
            assert gap % 4 == 0 or d16.data.stride(0) % 4 != 0
            if off:
                assert d16.data.data_ptr() % 8 != 0
            got = la.fit_instances(d16, masks, K, **{k: v for k, v in kw.items() if v is not None})
            check_oracle(got, up, masks, K, f"stride +{gap}, base +{off} {W}x{H} [{vid}]", ground=g)
            np.testing.assert_array_equal(np_(got[1]), np_(dense[1]))
            np.testing.assert_array_equal(np_(got[2])[:, 1:3], np_(dense[2])[:, 1:3])
        # one shared plane (plane_stride 0), as (H,W) and as (1,H,W)
        for shared in (stored[2], stored[2:3]):
            got = la.fit_instances(dev16(la, shared, variant), masks, K, **{k: v for k, v in kw.items() if v is not None})
            both_rules(la, got, up[2], kw, masks, K, f"shared plane {W}x{H} [{vid}]")


@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
@pytest.mark.parametrize("entry", ["rle", "poly", "bits"])
def test_frame_width_smaller_than_the_stored_width(la, entry, variant, vid):
    """rows padded by the caller (frame_width < W): the planes are 224 wide in memory, the image 214; the padding holds a sentinel
    outside every mask"""
    rs = np.random.RandomState(9)
    B, H, W, Wp = 8, 100, 214, 224
    segs = DC.ellipse_segs(rs, B, H, W) if entry == "poly" else None
    masks = (np.stack([DC.P.create_boolean_mask_from_polygon((W, H), s)[0] for s in segs]).astype(bool) if segs else DC.blob_masks(rs, B, H, W))
    stored = DC.quantise(DC.smooth_depth(rs, B, H, W), variant[0], variant[1])
    up = DC.upconvert(stored, variant[1], variant[2])
    wide = np.full((B, H, Wp), 60000.0 if variant[0] == "f16" else 65535, stored.dtype)
    wide[:, :, :W] = stored
    for g in (None, DC.ground_rows(rs, B)):
        kw = dict(ground=g)
        kk = {k: v for k, v in kw.items() if v is not None}
        got = fit(la, entry, dev16(la, wide, variant, frame_width=W), masks, DC.K224, segs=segs, **kk)
        both_rules(la, got, up, kw, masks, DC.K224, f"frame_width {entry} [{vid}]", entry, segs)
        unpadded = fit(la, entry, dev16(la, stored, variant), masks, DC.K224, segs=segs, **kk)   # padded by the wrapper: the same walk
        for a, b in zip(got, unpadded):
            np.testing.assert_array_equal(np_(a), np_(b))
    np.testing.assert_array_equal(np_(la.unpack_depth16(dev16(la, wide, variant, frame_width=W))), up)


# ------------------------------------------------------------------------------------------
# 5. batch sizes, area_hint, engine pins
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
@pytest.mark.parametrize("B", [1, 3, 200, 300])
def test_batch_sizes_area_hint_and_pins(la, B, variant, vid, monkeypatch):
    """1 / 3 / 200 / 300 instances at 96 x 224: the ranges in which float32 calls pick the row / band / split engines, and the
    size-balanced launch order above 256; a 16-bit call runs on the instance engine whatever is pinned"""
    rs = np.random.RandomState(50 + B)
    H, W, Pn = 96, 224, min(B, 5)
    masks = np.zeros((B, H, W), bool)
    vv, uu = np.mgrid[0:H, 0:W]
    for n in range(B):
        cy, cx, ry, rx = rs.uniform(0.2, 0.8) * H, rs.uniform(0.2, 0.8) * W, rs.uniform(0.05, 0.45) * H, rs.uniform(0.05, 0.45) * W
        masks[n] = ((vv - cy) / ry) ** 2 + ((uu - cx) / rx) ** 2 <= 1.0
    stored = DC.quantise(DC.smooth_depth(rs, Pn, H, W), variant[0], variant[1])
    up = DC.upconvert(stored, variant[1], variant[2])
    ii = (np.arange(B) % Pn).astype(np.int32)
    d16 = dev16(la, stored, variant)
    for g in (None, DC.ground_rows(rs, B)):
        kw = dict(ground=g, image_index=ii)
        kk = {k: v for k, v in kw.items() if v is not None}
        got = la.fit_instances(d16, masks, DC.K224, **kk)
        status = both_rules(la, got, up, kw, masks, DC.K224, f"B={B} [{vid}]")
        assert (status == 0).all()
        want = [np_(t) for t in got]
        for engine in ("rows", "band", "split", "instance"):       # pins give way: the same records, bit for bit
            monkeypatch.setattr(SCHED(), "engine", engine)
            for a, b in zip(want, la.fit_instances(d16, masks, DC.K224, **kk)):
                np.testing.assert_array_equal(a, np_(b), err_msg=f"pinned {engine}")
        monkeypatch.setattr(SCHED(), "engine", None)
        # area_hint given / absent, launch order on / off: records never depend on either
        rles = [O.rle_encode(m) for m in masks]
        areas = masks.reshape(B, -1).sum(1).astype(np.int32)
        base = la.fit_instances_ex(d16, DC.K224, rles=rles, **kk)
        for hint, order in ((areas, None), (areas[::-1].copy(), True), (None, False), (None, True)):
            monkeypatch.setattr(SCHED(), "launch_order", order)
            r = la.fit_instances_ex(d16, DC.K224, rles=rles, area_hint=hint, **kk)
            for key in ("boxes", "status", "aux"):
                np.testing.assert_array_equal(np_(r[key]), np_(base[key]), err_msg=f"area_hint {hint is not None}, order {order}")
        monkeypatch.setattr(SCHED(), "launch_order", None)
        both_rules(la, (base["boxes"], base["status"], base["aux"]), up, kw, masks, DC.K224, f"rle B={B} [{vid}]", "rle")


# ------------------------------------------------------------------------------------------
# 6. packers
# ------------------------------------------------------------------------------------------
def packer_input(rs, Pn, H, W):
    d = rs.uniform(0.0, 12.0, (Pn, H, W)).astype(np.float32)
    flat = d.reshape(-1)
    flat[::17] = np.nan
    flat[3::29] = np.inf
    flat[5::31] = -np.inf
    flat[7::13] = -1.5
    flat[11::19] = 0.0
    flat[2::23] = -0.0
    flat[4::37] = 70.0          # above 65.535 m: saturates at 65535 units of 1 mm
    flat[6::41] = 65519.9       # rounds to 65504 as float16
    flat[8::43] = 65520.0       # rounds to inf as float16
    flat[9::47] = 6e-8          # a float16 subnormal
    flat[10::53] = 2e-8         # below half the smallest subnormal: 0
    flat[12::59] = 0.0005       # exactly half a unit at 1 mm: rint goes to even
    flat[14::61] = 0.0015
    return d


@pytest.mark.parametrize("H,W", [(96, 224), (61, 75), (37, 53), (8, 32)])
def test_pack_and_unpack_depth16(la, H, W):
    import torch

    rs = np.random.RandomState(H * 3 + W)
    Pn = 5
    d = packer_input(rs, Pn, H, W)
    Wp = (W + 31) // 32 * 32
    for dtype, scale in (("f16", 1.0), ("u16", 0.001), ("u16", 0.00025)):
        want = DC.quantise(d, dtype, scale)
        tdt = torch.float16 if dtype == "f16" else torch.uint16
        for src in (d, torch.as_tensor(d, device="cuda")):
            p = la.pack_depth16(src, dtype, scale)
            assert p.data.dtype == tdt and tuple(p.data.shape) == (Pn, H, W) and p.frame_width == 0 and p.zero_is_hole
            assert p.scale == (scale if dtype == "u16" else 1.0)
            np.testing.assert_array_equal(np_(p.data.view(torch.int16)), want.view(np.int16), err_msg=f"{dtype} {scale}")
        p2 = la.pack_depth16(d[1], dtype, scale)                      # one (H,W) plane
        assert tuple(p2.data.shape) == (H, W)
        np.testing.assert_array_equal(np_(p2.data.view(torch.int16)), want[1].view(np.int16))
        pp = la.pack_depth16(d, dtype, scale, frame_pad=True)          # rows padded with zeros
        assert tuple(pp.data.shape) == (Pn, H, Wp) and pp.frame_width == (W if Wp != W else 0)
        got = np_(pp.data.view(torch.int16))
        np.testing.assert_array_equal(got[:, :, :W], want.view(np.int16))
        assert (got[:, :, W:] == 0).all()
        # strided input planes, a base one element into an allocation
        big = torch.zeros((2 * Pn, H, W), dtype=torch.float32, device="cuda")
        big[::2] = torch.as_tensor(d, device="cuda")
        np.testing.assert_array_equal(np_(la.pack_depth16(big[::2], dtype, scale).data.view(torch.int16)), want.view(np.int16))
        # an `out` with a wider plane stride: what lies between two planes stays untouched
        for extra, off in ((8, 0), (3, 1)):
            flat = torch.full((off + Pn * (H * W + extra) + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
            out = torch.as_strided(flat.view(tdt), (Pn, H, W), (H * W + extra, W, 1), off)
            r = la.pack_depth16(d, dtype, scale, out=out)
            assert r.data.data_ptr() == out.data_ptr()
            f = np_(flat)
            body = np.lib.stride_tricks.as_strided(f[off:], (Pn, H * W), (2 * (H * W + extra), 2))
            np.testing.assert_array_equal(body.reshape(Pn, H, W), want.view(np.int16))
            gapw = np.lib.stride_tricks.as_strided(f[off + H * W:], (Pn, extra), (2 * (H * W + extra), 2))
            assert (gapw == 0x5A5A).all() and (f[:off] == 0x5A5A).all(), "words between two planes were written"
            # ... and unpack reads such planes where they lie
            for hole in (True, False):
                np.testing.assert_array_equal(np_(la.unpack_depth16(r._replace(zero_is_hole=hole))), DC.upconvert(want, scale, hole))
        # unpack: the value rule
        for hole in (True, False):
            back = la.unpack_depth16(dev16(la, want, (dtype, scale, hole)))
            assert back.dtype == torch.float32 and tuple(back.shape) == (Pn, H, W)
            np.testing.assert_array_equal(np_(back), DC.upconvert(want, scale, hole))
        np.testing.assert_array_equal(np_(la.unpack_depth16(pp)), DC.upconvert(want, scale, True))   # padded: the image columns
    # every 16-bit word through unpack: the whole value table of either format
    allw = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    np.testing.assert_array_equal(np_(la.unpack_depth16(dev16(la, allw.view(np.float16), ("f16", 1.0, True)))).view(np.uint32) & 0xff800000,
                                  allw.view(np.float16).astype(np.float32).view(np.uint32) & 0xff800000)
    fin = np.isfinite(allw.view(np.float16))
    np.testing.assert_array_equal(np_(la.unpack_depth16(dev16(la, allw.view(np.float16), ("f16", 1.0, True))))[fin], allw.view(np.float16).astype(np.float32)[fin])
    for scale in (0.001, 0.00025, 1.0, 3.3e-5):
        np.testing.assert_array_equal(np_(la.unpack_depth16(dev16(la, allw, ("u16", scale, True)))), DC.upconvert(allw, scale, True))


@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
def test_fit_of_packed_equals_fit_of_numpy_quantised(la, variant, vid):
    rs = np.random.RandomState(12)
    B, H, W = 8, 100, 214
    masks = DC.blob_masks(rs, B, H, W)
    d = DC.smooth_depth(rs, B, H, W)
    d[0][masks[0] & (rs.rand(H, W) < 0.05)] = np.nan                  # holes: NaN stays NaN (float16), becomes a stored 0 (uint16)
    stored = DC.quantise(d, variant[0], variant[1])
    ground = DC.ground_rows(rs, B)
    for g in (None, ground):
        kk = {} if g is None else dict(ground=g)
        want = la.fit_instances(dev16(la, stored, variant), masks, DC.K224, **kk)
        packed = la.pack_depth16(d, variant[0], variant[1])._replace(zero_is_hole=variant[2])
        for a, b in zip(la.fit_instances(packed, masks, DC.K224, **kk), want):
            np.testing.assert_array_equal(np_(a), np_(b))
        rles = [O.rle_encode(m) for m in masks]
        want = la.fit_instances_rle(dev16(la, stored, variant), rles, DC.K224, **kk)
        padded = la.pack_depth16(d, variant[0], variant[1], frame_pad=True)._replace(zero_is_hole=variant[2])
        assert padded.frame_width == W and padded.data.shape[-1] == 224
        for a, b in zip(la.fit_instances_rle(padded, rles, DC.K224, **kk), want):
            np.testing.assert_array_equal(np_(a), np_(b))
    assert (np_(want[1])[:B - 1] == 0).all()


# ------------------------------------------------------------------------------------------
# 7. streams, graphs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
def test_side_stream_behind_the_upload(la, variant, vid):
    import torch

    rs = np.random.RandomState(30)
    B, H, W = 12, 96, 224
    masks = DC.blob_masks(rs, B, H, W)
    stored = DC.quantise(DC.smooth_depth(rs, B, H, W), variant[0], variant[1])
    up = DC.upconvert(stored, variant[1], variant[2])
    side = torch.cuda.Stream()
    d16 = dev16(la, stored, variant)                                 # uploaded on the current stream; the call is ordered behind it
    got = la.fit_instances(d16, masks, DC.K224, stream=side)
    side.synchronize()
    both_rules(la, got, up, {}, masks, DC.K224, f"side stream [{vid}]")
    got = la.fit_instances_bits(d16, host_bits(masks), DC.K224, stream=side)
    side.synchronize()
    both_rules(la, got, up, {}, masks, DC.K224, f"side stream bits [{vid}]", "bits")


@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
@pytest.mark.parametrize("method", ["pca", "convex_hull"])
def test_run_captured_into_a_graph(la, method, variant, vid):
    """InstanceFitter.run with a Depth16: one launch (two for a hull call) in a linear chain, captured once, replayed on refilled inputs"""
    import torch

    from labelany3d_amd import InstanceFitter

    B, H, W = 300, 96, 224
    dev = torch.device("cuda", 0)
    K = np.array([[0.8 * W, 0, W / 2.0], [0, 0.8 * W, H / 2.0], [0, 0, 1]])

    def scene(seed):
        rs = np.random.RandomState(seed)
        return DC.quantise(DC.smooth_depth(rs, B, H, W), variant[0], variant[1]), DC.hull_masks(rs, B, H, W)

    stored0, masks0 = scene(17)
    d16 = dev16(la, stored0, variant)
    m = torch.as_tensor(masks0.view(np.uint8), device=dev)
    k = torch.as_tensor(K, device=dev)
    f = InstanceFitter(B, H, W, dev, method=method)
    side = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        f.run(d16, m, k, stream=side)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            f.run(d16, m, k, stream=torch.cuda.current_stream())
    fr = InstanceFitter(B, H, W, dev, method=method)
    for seed in (18, 19):
        stored1, masks1 = scene(seed)
        d16.data.view(torch.int16).copy_(torch.as_tensor(np.ascontiguousarray(stored1).view(np.int16), device=dev))
        m.copy_(torch.as_tensor(masks1.view(np.uint8), device=dev))
        f.boxes.fill_(12345.0); f.status.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        rb, rs_, ra = fr.run(d16, m, k)
        torch.cuda.synchronize()
        assert torch.equal(f.status[0], rs_) and (rs_ == 0).all()
        assert torch.equal(f.boxes[0], rb) and torch.equal(f.aux[0], ra)
        up = DC.upconvert(stored1, variant[1], variant[2])
        ub, us, ua = (t.clone() for t in fr.run(torch.as_tensor(up, device=dev), m, k, engine="instance"))
        torch.cuda.synchronize()
        same_engine((f.boxes[0], f.status[0], f.aux[0]), (ub, us, ua), f"graph replay vs float32 [{vid}]")
        if method == "pca":
            check_oracle((f.boxes[0], f.status[0], f.aux[0]), up, masks1, K, f"graph replay [{vid}]")
    with pytest.raises(ValueError, match="do not match"):
        f.run(la.Depth16(d16.data[:, :, :192]), m, k)


# ------------------------------------------------------------------------------------------
# 8. seeded randomised sweep
# ------------------------------------------------------------------------------------------
SWEEP_SHAPES = [(96, 224), (100, 224), (64, 96), (100, 214), (61, 75)]


@pytest.mark.parametrize("chunk", range(4))
def test_randomised_sweep(la, chunk):
    """4 x 10 seeded cases, none skipped: shape, dtype, scale, mask source, ground, subsample and hull drawn at random; both rules"""
    rs = np.random.RandomState(7000 + chunk)
    n_ok = n_all = 0
    for case in range(10):
        H, W = SWEEP_SHAPES[rs.randint(len(SWEEP_SHAPES))]
        dtype = ("f16", "u16")[rs.randint(2)]
        variant = (dtype, 1.0 if dtype == "f16" else float(rs.choice([0.001, 0.00025, 0.0005, 0.000125 * 3])), bool(rs.randint(2)))
        B = int(rs.randint(1, 9))
        shared = B > 1 and rs.rand() < 0.4
        Pn = int(rs.randint(1, min(B, 3) + 1)) if shared else B
        hull = rs.rand() < 0.3
        sample = rs.rand() < (0.6 if hull else 0.3)
        entry = ("u8", "rle", "poly", "bits")[rs.randint(4)]
        if hull and not sample and (entry == "poly" or (entry == "u8" and W % 32 != 0)):
            entry = "rle"                                             # (full-mask hull: masks that leave room for the column arrays)
        segs = None
        if entry == "poly":
            segs = DC.ellipse_segs(rs, B, H, W)
            masks = np.stack([DC.P.create_boolean_mask_from_polygon((W, H), s)[0] for s in segs]).astype(bool)
        elif hull and not sample:
            masks = DC.hull_masks(rs, B, H, W, rmax=0.16)
        else:
            masks = DC.blob_masks(rs, B + 3, H, W)[rs.permutation(B + 3)[:B]]
        gkind = 0 if (hull and not sample) else rs.randint(2)
        ground = DC.ground_rows(rs, B) if gkind else None
        K = np.array([[rs.uniform(120, 400), 0, W / 2 + rs.uniform(-5, 5)], [0, rs.uniform(120, 400), H / 2 + rs.uniform(-5, 5)], [0, 0, 1]])
        if not hull and rs.rand() < 0.2:
            K[0, 1] = rs.uniform(-3, 3)
        d = DC.smooth_depth(rs, Pn, H, W)
        if rs.rand() < 0.4:                                           # holes: NaN in float16, a stored 0 in uint16
            d[rs.rand(Pn, H, W) < 0.02] = np.nan
        stored = DC.quantise(d, variant[0], variant[1])
        up = DC.upconvert(stored, variant[1], variant[2])
        ii = rs.randint(0, Pn, B).astype(np.int32) if shared else None
        sidx = DC.draw_sample_idx(masks.reshape(B, -1).sum(1), rs) if sample else None
        method = "convex_hull" if hull else "pca"
        if hull and not sample and (H, W) in ((64, 96), (61, 75)):
            method = "pca"                                            # (fewer than 64 tiles: full-mask hull refuses the whole frame)
        kw = dict(ground=ground, sample_idx=sidx, image_index=ii)
        tag = f"chunk {chunk} case {case}: {entry} {variant} B={B} {W}x{H} planes={Pn} ground={ground is not None} sample={sample} {method}"
        got = fit(la, entry, dev16(la, stored, variant), masks, K, segs=segs, method=method, **{k: v for k, v in kw.items() if v is not None})
        status = both_rules(la, got, up, kw, masks, K, tag, entry, segs, method)
        n_ok += int((status == 0).sum()); n_all += B
    print(f"sweep chunk {chunk}: {n_ok} of {n_all} instances fitted (status 0)")
    assert 2 * n_ok >= n_all
