"""GPU tests of the frames call (include/la3d.h "images of different sizes in one call"; ``pack_frames`` / ``fit_instances_frames``):
one call over images of several sizes against the oracle run image by image on the UNPADDED frames, against the uniform entry run
size group by size group, the on-device contract checks, the call-level refusals, a seeded sweep over the campaign generators'
mask shapes, and ``ScenePipeline(mixed_frames=True)`` against the default mode.

Bounds.  Against the oracle, records, 2-D boxes and yaw are held to rtol = atol = 1e-9 (the figure of the suite's GPU tests) and
status / n_in / n_valid / filter statistics are equal; the inputs of those tests are chosen well conditioned (and checked on the
CPU first: the oracle fits every instance with status 0 except the ones put there for their status).  Against the uniform entry:
status, aux[:, 1:3] and statistics equal, records to 1e-9 (engines differ by batch size) - and to 1e-12 when all frames have one
size and both calls are pinned to the instance engine (the two-entry rule of tests/test_gpu_bits.py::same_engine).  The sweep
goes through degenerate masks (one pixel, one row, constant depth ...): it uses the campaign's own rule (oracle/campaigns/
engines.py::check_run: ``assert_records`` with the eigen-gap conditioning; an exact tie of the eigenvalues - gap < 1e-9, the
documented "any yaw is as good" - is compared in status, n_in and n_valid, not in its axis)."""
import json

import numpy as np
import pytest

from oracle import la3d_oracle as O
from oracle.campaigns import engines as CE

from .conftest import SCHED
from .test_gpu_parity import assert_records, reference_axis_noise

pytestmark = pytest.mark.gpu

SIZES = [(480, 640), (640, 480), (427, 640), (375, 500), (500, 333), (96, 224)]   # (H, W): pitches 640, 480, 640, 512, 352, 224


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def np_(t):
    return t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()


def ellipse_polygon(rs, H, W):
    """a polygon annotation like the COCONut converter writes (outline of an ellipse, half-pixel coordinates, sometimes two parts)
    and the mask the reference's cv2.fillPoly gives for it"""
    from oracle import poly_oracle as P

    hh, ww = rs.uniform(0.15, 0.6) * H, rs.uniform(0.15, 0.6) * W
    cy, cx = rs.uniform(0.25, 0.75) * H, rs.uniform(0.25, 0.75) * W
    ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
    px, py = np.round((cx + ww / 2 * np.cos(ang)) * 2) / 2, np.round((cy + hh / 2 * np.sin(ang)) * 2) / 2
    seg = [np.stack([px, py], 1).reshape(-1).tolist()]
    if rs.rand() < 0.4:
        seg.append((np.stack([px, py], 1) * [0.5, 0.6] + [W * 0.45, H * 0.35]).reshape(-1).tolist())   # (reaches past the frame for some)
    m, _ = P.create_boolean_mask_from_polygon((W, H), seg)
    return m, seg


def blob(rs, H, W, k):
    m = np.zeros((H, W), bool)
    if k % 3 == 0:
        h, w = rs.randint(H // 6, H // 2), rs.randint(W // 6, W // 2)
        r0, c0 = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
        m[r0:r0 + h, c0:c0 + w] = True
    elif k % 3 == 1:
        vv, uu = np.mgrid[0:H, 0:W]
        m = ((uu - rs.uniform(0.3, 0.7) * W) / (rs.uniform(0.1, 0.3) * W)) ** 2 + ((vv - rs.uniform(0.3, 0.7) * H) / (rs.uniform(0.1, 0.3) * H)) ** 2 < 1.0
    else:
        m = rs.rand(H, W) < 0.02
        m[:, W - 3:] |= rs.rand(H, 3) < 0.5          # pixels in the LAST columns of the unpadded frame
    return m


def make_mix(seed, sizes=SIZES, per_image=4, poly=False, empty_image=2, special=True):
    """images of the given sizes (one without instances), ``per_image`` instances each, as masks (+ polygon parts)"""
    rs = np.random.RandomState(seed)
    P = len(sizes)
    depth = [rs.uniform(0.5, 10, s).astype(np.float32) for s in sizes]
    K = np.stack([np.array([[rs.uniform(0.7, 1.3) * w, 0, w / 2 + rs.uniform(-9, 9)], [0, rs.uniform(0.7, 1.3) * w, h / 2 + rs.uniform(-9, 9)], [0, 0, 1]])
                  for h, w in sizes])
    masks, segs, img = [], [], []
    for p, (h, w) in enumerate(sizes):
        if p == empty_image:
            continue
        for k in range(per_image):
            if poly:
                m, seg = ellipse_polygon(rs, h, w)
                segs.append(seg)
            else:
                m = blob(rs, h, w, k + p)
            masks.append(m); img.append(p)
    expect = np.zeros(len(masks), np.int32)
    if special and not poly:   # two instances that are there for their status
        masks[1] = np.zeros_like(masks[1]); expect[1] = 1                       # empty: no valid points
        masks[5] = np.zeros_like(masks[5]); masks[5][3, 4] = True; expect[5] = 3   # one pixel: too few points
    return dict(sizes=list(sizes), depth=depth, K=K, masks=masks, segs=segs if poly else None, img=np.asarray(img, np.int32), expect=expect)


def shuffled(mix, seed):
    """the same instances in a shuffled order (image_index no longer sorted)"""
    order = np.random.RandomState(seed).permutation(len(mix["masks"]))
    out = dict(mix)
    out["masks"] = [mix["masks"][i] for i in order]
    out["segs"] = None if mix["segs"] is None else [mix["segs"][i] for i in order]
    out["img"], out["expect"] = mix["img"][order], mix["expect"][order]
    return out


def oracle_mix(mix, ground=None, sidx=None, kappa=False):
    """the oracle image by image, on the unpadded frames"""
    B = len(mix["masks"])
    rec, st, yaw, nv, kap = np.full((B, 39), np.nan), np.zeros(B, np.int32), np.full(B, np.nan), np.zeros(B, np.int64), np.full(B, np.nan)
    for p in range(len(mix["sizes"])):
        sel = np.flatnonzero(mix["img"] == p)
        if not len(sel):
            continue
        g = None if ground is None else [None if np.isnan(ground[i][0]) else ground[i] for i in sel]
        r, s, y, n, k = O.fit_instances(mix["depth"][p], np.stack([mix["masks"][i] for i in sel]), mix["K"][p], ground=g,
                                        sample_idx=None if sidx is None else sidx[sel], return_kappa=True)
        rec[sel], st[sel], yaw[sel], nv[sel], kap[sel] = r, s, y, n, k
    return (rec, st, yaw, nv, kap) if kappa else (rec, st, yaw, nv)


def frames_call(la, mix, pf=None, **kw):
    pf = la.pack_frames(mix["depth"]) if pf is None else pf
    if mix["segs"] is not None:
        src = dict(polys=la.pack_polygons(mix["segs"], pf.H, pf.W))
    else:
        src = dict(rles=[O.rle_encode(m) for m in mix["masks"]])
    res = la.fit_instances_frames(pf, mix["K"], image_index=mix["img"], **src, **kw)
    return {k: np_(v) for k, v in res.items()}


def grouped_call(la, mix, engine=None, **kw):
    """the same instances through the uniform entry, one call per frame size (what a caller had to do before)"""
    B = len(mix["masks"])
    out = dict(boxes=np.full((B, 39), np.nan), status=np.full(B, -1, np.int32), aux=np.full((B, 4), np.nan), stats=np.zeros((B, 4), np.int32),
               boxes2d=np.full((B, 8), np.nan))
    per = {k: kw.pop(k) for k in ("ground", "sample_idx") if k in kw}
    proj = kw.pop("proj", False)
    SCHED().engine = engine
    try:
        for size in sorted(set(mix["sizes"])):
            imgs = [p for p, s in enumerate(mix["sizes"]) if s == size]
            sel = np.flatnonzero(np.isin(mix["img"], imgs))
            if not len(sel):
                continue
            local = np.asarray([imgs.index(int(mix["img"][i])) for i in sel], np.int32)
            src = (dict(polys=la.pack_polygons([mix["segs"][i] for i in sel], size[0], size[1])) if mix["segs"] is not None
                   else dict(rles=[O.rle_encode(mix["masks"][i]) for i in sel]))
            res = la.fit_instances_ex(np.stack([mix["depth"][p] for p in imgs]), mix["K"][imgs], image_index=local,
                                      image_size=(size[1], size[0]) if proj else None,
                                      **{k: (None if v is None else np.asarray(v)[sel]) for k, v in per.items()}, **src, **kw)
            out["boxes"][sel], out["status"][sel], out["aux"][sel] = np_(res["boxes"]), np_(res["status"]), np_(res["aux"])
            if "stats" in res:
                out["stats"][sel] = np_(res["stats"])
            if proj:
                out["boxes2d"][sel] = np_(res["boxes2d"])
    finally:
        SCHED().engine = None
    return out


def check_strict(got, mix, ref, tag, expect=None):
    """status / n_in / n_valid equal; records and yaw within rtol = atol = 1e-9 of the oracle"""
    rec, st, yaw, nv = ref
    expect = st if expect is None else expect
    np.testing.assert_array_equal(got["status"], expect, err_msg=f"{tag} status")
    ok = expect == 0
    assert np.isnan(got["boxes"][~ok]).all(), f"{tag}: a rejected instance's record is not NaN"
    fitted = expect != 6          # (a filtered instance reports its area in aux[2] too, and no n_valid)
    np.testing.assert_array_equal(got["aux"][:, 2], [m.sum() for m in mix["masks"]], err_msg=f"{tag} n_in")
    np.testing.assert_array_equal(got["aux"][ok, 1], nv[ok], err_msg=f"{tag} n_valid")
    assert fitted.any()
    d = np.abs(got["boxes"][ok] - rec[ok])
    print(f"{tag}: {int(ok.sum())} of {len(ok)} fitted; max |record - oracle| {d.max():.3g}, max |yaw - oracle| {np.abs(got['aux'][ok, 0] - yaw[ok]).max():.3g}, "
          f"smallest eigen-gap {got['aux'][ok, 3].min():.3g}")
    np.testing.assert_allclose(got["boxes"][ok], rec[ok], rtol=1e-9, atol=1e-9, err_msg=f"{tag} records")
    np.testing.assert_allclose(got["aux"][ok, 0], yaw[ok], rtol=1e-9, atol=1e-9, err_msg=f"{tag} yaw")


def ground_rows(B, seed, some_nan=True):
    rs = np.random.RandomState(seed)
    g = np.array([[0.02, -0.98, 0.1, 1.5]] * B) + 0.03 * rs.randn(B, 4)
    if some_nan:
        g[rs.rand(B) < 0.3, 0] = np.nan          # "no ground" for these instances
    return g


def draws(mix, seed):
    rs = np.random.RandomState(seed)
    counts = np.asarray([m.sum() for m in mix["masks"]])
    idx = np.zeros((len(counts), 500), np.int32)
    for n, c in enumerate(counts):
        if c > 500:
            idx[n] = rs.randint(0, int(c), 500)
    return idx


# ------------------------------------------------------------------------------------------
# 1. one mixed call against the oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poly", [False, True], ids=["rle", "poly"])
@pytest.mark.parametrize("sample", [False, True], ids=["full", "subsample"])
@pytest.mark.parametrize("grounded", [False, True], ids=["no-ground", "ground"])
def test_mixed_batch_against_oracle(la, poly, sample, grounded):
    mix = make_mix(11 + poly, poly=poly)
    assert len(set(mix["sizes"])) >= 6 and not (mix["img"] == 2).any()        # six sizes, one image without instances
    B = len(mix["masks"])
    ground = ground_rows(B, 5) if grounded else None
    sidx = draws(mix, 6) if sample else None
    ref = oracle_mix(mix, ground, sidx)
    np.testing.assert_array_equal(ref[1], mix["expect"], err_msg="the oracle does not fit the chosen inputs as planned")   # on the CPU, first
    assert (ref[1] == 0).sum() >= B - 2
    tag = f"{'poly' if poly else 'rle'} {'subsample' if sample else 'full'} {'ground' if grounded else 'no ground'}"
    got = frames_call(la, mix, ground=ground, sample_idx=sidx)
    check_strict(got, mix, ref, tag)
    # the same instances in a shuffled order: every record follows its instance
    perm = shuffled(mix, 3)
    order = np.random.RandomState(3).permutation(B)
    got_s = frames_call(la, perm, ground=None if ground is None else ground[order], sample_idx=None if sidx is None else sidx[order])
    check_strict(got_s, perm, tuple(v[order] for v in ref), tag + " shuffled")
    np.testing.assert_array_equal(got_s["boxes"], got["boxes"][order])
    np.testing.assert_array_equal(got_s["aux"], got["aux"][order])


@pytest.mark.parametrize("poly", [False, True], ids=["rle", "poly"])
def test_mixed_batch_filter_stats_and_proj(la, poly):
    """the fused filter with statistics, and the 2-D boxes clamped to each instance's OWN frame"""
    mix = make_mix(21 + poly, poly=poly, special=False)
    B = len(mix["masks"])
    rec, st, yaw, nv = oracle_mix(mix)
    assert (st == 0).all()
    for flt in (True, {"boundary_threshold": 3, "scale_threshold": 400}):
        b, a = (10, 100) if flt is True else (3, 400)
        stats = np.array([O.mask_stats(m, b) for m in mix["masks"]])
        keep = np.array([O.keep_instance(s, mix["sizes"][p][0], not poly, a) for s, p in zip(stats, mix["img"])])
        assert keep.any() and (~keep).any(), "the inputs should exercise both sides of the keep rule"
        got = frames_call(la, mix, filter=flt, proj=True)
        np.testing.assert_array_equal(got["stats"], stats, err_msg="filter statistics")
        expect = np.where(keep, st, 6).astype(np.int32)
        check_strict(got, mix, (rec, st, yaw, nv), f"filter {flt}", expect=expect)
        ok = expect == 0
        want2d = np.stack([O.project_boxes(rec[i:i + 1], mix["K"][mix["img"][i]], (mix["sizes"][mix["img"][i]][1], mix["sizes"][mix["img"][i]][0]))[0]
                           for i in range(B)])
        assert np.isfinite(want2d[ok]).all()
        np.testing.assert_allclose(got["boxes2d"][ok], want2d[ok], rtol=1e-9, atol=1e-9, err_msg="2-D boxes")
        assert np.isnan(got["boxes2d"][~ok]).all()
        # some box is actually clamped by its own frame's width / height (and not by the bounds of the call)
        clamp_w = np.asarray([mix["sizes"][p][1] for p in mix["img"]], float)
        clamp_h = np.asarray([mix["sizes"][p][0] for p in mix["img"]], float)
        assert (got["boxes2d"][ok, 6] <= clamp_w[ok]).all() and (got["boxes2d"][ok, 7] <= clamp_h[ok]).all()


# ------------------------------------------------------------------------------------------
# 2. the same instances, grouped by size, through the uniform entry
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poly", [False, True], ids=["rle", "poly"])
@pytest.mark.parametrize("mode", ["plain", "ground", "subsample", "filter"])
def test_same_instances_grouped_by_size(la, poly, mode):
    mix = make_mix(31 + poly, poly=poly)
    B = len(mix["masks"])
    kw = {}
    if mode == "ground":
        kw["ground"] = ground_rows(B, 8)
    if mode == "subsample":
        kw["sample_idx"] = draws(mix, 9)
    if mode == "filter":
        kw.update(filter=True, proj=True)
    got = frames_call(la, mix, **kw)
    want = grouped_call(la, mix, **kw)
    np.testing.assert_array_equal(got["status"], want["status"])
    np.testing.assert_array_equal(got["aux"][:, 1:3], want["aux"][:, 1:3])
    if mode == "filter":
        np.testing.assert_array_equal(got["stats"], want["stats"])
        np.testing.assert_allclose(np.nan_to_num(got["boxes2d"], nan=-7.0), np.nan_to_num(want["boxes2d"], nan=-7.0), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(np.nan_to_num(got["boxes"], nan=-7.0), np.nan_to_num(want["boxes"], nan=-7.0), rtol=1e-9, atol=1e-9)
    assert (got["status"] == 0).sum() >= B // 2


# ------------------------------------------------------------------------------------------
# 3. one frame size only: the frames entry against the uniform entry on the same engine
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(480, 640), (375, 500), (96, 224)])
@pytest.mark.parametrize("poly", [False, True], ids=["rle", "poly"])
def test_one_frame_size_equals_uniform_entry(la, size, poly):
    mix = make_mix(41 + poly, sizes=[size] * 5, per_image=5, poly=poly, empty_image=3)
    B = len(mix["masks"])
    for mode, kw in (("plain", {}), ("ground", dict(ground=ground_rows(B, 4))), ("subsample", dict(sample_idx=draws(mix, 2))),
                     ("filter", dict(filter=True))):
        got = frames_call(la, mix, **kw)
        want = grouped_call(la, mix, engine="instance", **kw)
        np.testing.assert_array_equal(got["status"], want["status"], err_msg=mode)
        np.testing.assert_array_equal(got["aux"][:, 1:3], want["aux"][:, 1:3], err_msg=mode)
        if mode == "filter":
            np.testing.assert_array_equal(got["stats"], want["stats"])
        np.testing.assert_allclose(np.nan_to_num(got["boxes"], nan=-7.0), np.nan_to_num(want["boxes"], nan=-7.0), rtol=1e-12, atol=1e-12, err_msg=mode)
        assert (got["status"] == 0).sum() >= (1 if mode == "filter" else B // 2)   # (the keep rule drops most masks of a small frame)


# ------------------------------------------------------------------------------------------
# 4. contract breaks are answered per instance, on the device
# ------------------------------------------------------------------------------------------
def test_contract_breaks_get_status_5(la):
    """Frame rows that break the contract (and image indices outside the table): their instances get status 5 and NaN, every other
    instance of the call is fitted exactly as in the clean call.  Nothing is provoked: the kernel decides before it forms an address
    from a broken row, and every broken row here would - were it read all the same - still address floats INSIDE the depth buffer
    (the broken rows belong to the small images at the front of the buffer, the large ones lie behind them)."""
    import torch

    sizes = [(64, 96), (96, 224), (100, 214), (37, 53), (120, 160), (480, 640), (427, 640)]
    mix = make_mix(51, sizes=sizes, per_image=3, empty_image=-1, special=False)
    B = len(mix["masks"])
    pf = la.pack_frames(mix["depth"])
    clean = frames_call(la, mix, pf=pf, filter=True, proj=True)
    ref = oracle_mix(mix)
    assert (ref[1] == 0).all()
    table = pf.table_host.copy()
    table["W"][0] = 48                                       # pitch not a multiple of 32 (frame_width 48 would fit it)
    table["frame_width"][0] = 48
    table["depth_offset"][1] += 2                            # plane not 16-byte aligned
    table["H"][2] = pf.H + 8                                 # more rows than the bound of the call
    table["frame_width"][3] = table["W"][3] + 1              # more image columns than the pitch
    table["W"][4] = pf.W + 32                                # a pitch above the bound of the call
    broken_imgs = [0, 1, 2, 3, 4]
    assert int(table["depth_offset"][4]) + (pf.H + 8) * (pf.W + 32) <= pf.depth.numel()
    words = torch.as_tensor(np.ascontiguousarray(table).view(np.int32).reshape(len(sizes), 6).copy(), device="cuda")
    bad = pf._replace(table=words, table_host=table)
    img = mix["img"].copy()
    img[-1], img[-2] = len(sizes), -1                        # image_index outside [0, P): both ends
    mixb = dict(mix, img=img)
    got = frames_call(la, mixb, pf=bad, filter=True, proj=True)
    broken = np.isin(mix["img"], broken_imgs)
    broken[-1] = broken[-2] = True
    assert broken.sum() >= 10 and (~broken).sum() >= 4
    np.testing.assert_array_equal(got["status"][broken], 5)
    assert np.isnan(got["boxes"][broken]).all() and np.isnan(got["boxes2d"][broken]).all() and np.isnan(got["aux"][broken][:, [0, 2, 3]]).all()
    for k in ("boxes", "status", "aux", "stats", "boxes2d"):
        np.testing.assert_array_equal(got[k][~broken], clean[k][~broken], err_msg=f"{k} of the instances on conforming frames")
    assert (got["status"][~broken] != 5).all()
    # negative offset, zero rows, zero frame_width: refused as well
    table2 = pf.table_host.copy()
    table2["depth_offset"][0] = -4
    table2["H"][1] = 0
    table2["frame_width"][2] = 0
    words2 = torch.as_tensor(np.ascontiguousarray(table2).view(np.int32).reshape(len(sizes), 6).copy(), device="cuda")
    got2 = frames_call(la, mix, pf=pf._replace(table=words2, table_host=table2))
    b2 = np.isin(mix["img"], [0, 1, 2])
    np.testing.assert_array_equal(got2["status"][b2], 5)
    np.testing.assert_array_equal(got2["boxes"][~b2], frames_call(la, mix, pf=pf)["boxes"][~b2])


# ------------------------------------------------------------------------------------------
# 5. call-level refusals, stream ordering, small frames, the launch order
# ------------------------------------------------------------------------------------------
def test_call_level_refusals(la):
    import ctypes as C

    import torch

    from labelany3d_amd import _lib

    mix = make_mix(61, sizes=[(64, 96), (96, 224)], per_image=2, empty_image=-1, special=False)
    pf = la.pack_frames(mix["depth"])
    with pytest.raises(ValueError, match="convex_hull"):
        frames_call(la, mix, pf=pf, method="convex_hull")
    B = len(mix["masks"])
    dev = pf.depth.device
    t = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)   # noqa: E731
    out, status, K, ws = t(B, 39), t(B, dt=torch.int32), torch.as_tensor(mix["K"], device=dev), t(1 << 16, dt=torch.uint8)
    ii = torch.as_tensor(mix["img"], device=dev)
    u8 = t(B, pf.H * pf.W, dt=torch.uint8)
    counts, offsets, _ = la.masks.pack_rle_frames([O.rle_encode(m) for m in mix["masks"]])
    c, o = torch.as_tensor(counts, device=dev), torch.as_tensor(offsets, device=dev)

    def call(**kw):
        a = _lib.FitArgs(struct_size=C.sizeof(_lib.FitArgs), B=B, H=pf.H, W=pf.W, depth=pf.depth.data_ptr(), K=K.data_ptr(), k_stride=9,
                         out=out.data_ptr(), status=status.data_ptr(), workspace=ws.data_ptr(), image_index=ii.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        rc = _lib.lib.la3d_fit_instances_frames(C.byref(a), pf.table.data_ptr(), len(mix["sizes"]))
        return rc, _lib.lib.la3d_last_error().decode()

    assert call(mask=u8.data_ptr())[0] == _lib.ERR_UNSUPPORTED                       # u8 planes
    rc, msg = call()                                                                 # what a bit-plane call hands over: no mask source in the block
    assert rc == -1 and "rle_counts / poly_xy" in msg                                # (the frames entry takes no bit planes)
    assert call(rle_counts=c.data_ptr(), rle_offsets=o.data_ptr(), method=_lib.METHOD_CONVEX_HULL)[0] == _lib.ERR_UNSUPPORTED
    status.fill_(-1)
    assert call(rle_counts=c.data_ptr(), rle_offsets=o.data_ptr())[0] == 0           # and the plain call through the C entry fits
    torch.cuda.synchronize()
    np.testing.assert_array_equal(np_(status), frames_call(la, mix, pf=pf)["status"])
    assert (np_(status) == 0).all()


def test_stream_ordering_and_pinned_engines(la):
    """the call is an enqueue on the caller's stream, ordered behind the uploads; engine pins and builds give way / change nothing"""
    import torch

    mix = make_mix(71, sizes=[(96, 224), (64, 96), (100, 214), (200, 320)], per_image=4, empty_image=-1)
    want = frames_call(la, mix)
    side = torch.cuda.Stream()
    got = frames_call(la, mix, stream=side)
    side.synchronize()
    for k in ("boxes", "status", "aux"):
        np.testing.assert_array_equal(got[k], want[k])
    for engine in ("rows", "band", "split", "instance"):
        SCHED().engine = engine
        try:
            g = frames_call(la, mix)
        finally:
            SCHED().engine = None
        for k in ("boxes", "status", "aux"):
            np.testing.assert_array_equal(g[k], want[k], err_msg=f"pinned {engine}")


def test_small_frames_are_fitted(la):
    """frames below 64 tiles of 32 x 8 pixels - alone in a call, and next to large ones - are fitted, not refused"""
    for sizes in ([(8, 32), (16, 32), (5, 7), (24, 48), (37, 53)], [(8, 32), (480, 640), (5, 7), (37, 53)]):
        mix = make_mix(81, sizes=sizes, per_image=2, empty_image=-1, special=False)
        for i, m in enumerate(mix["masks"]):          # whole-frame and half-frame masks: small frames, enough points
            m[:] = False
            m[: m.shape[0] // (1 + i % 2) or 1] = True
        ref = oracle_mix(mix, kappa=True)
        got = frames_call(la, mix)
        np.testing.assert_array_equal(got["status"], ref[1])
        assert (got["status"] != 5).all() and (got["status"] == 0).any()
        ok = (ref[1] == 0) & (got["aux"][:, 3] >= 1e-9)
        noise = reference_axis_noise(ref[4], got["aux"][:, 1], got["aux"][:, 3])
        assert_records(got["boxes"][ok], ref[0][ok], f"small frames {sizes}", gap=got["aux"][ok, 3], noise=noise[ok])


def test_launch_order_from_area_hint_is_invisible(la):
    """B above 256: with ``area_hint`` the size-balanced order runs (right, wrong and absurd hints), without it the plain order -
    the records are the same"""
    sizes = [(96, 224), (64, 96), (100, 214), (120, 160), (37, 53), (200, 320)]
    mix = make_mix(91, sizes=sizes, per_image=50, empty_image=-1, special=False)
    B = len(mix["masks"])
    assert B > 256
    pf = la.pack_frames(mix["depth"])
    want = frames_call(la, mix, pf=pf)
    areas = np.asarray([m.sum() for m in mix["masks"]], np.int32)
    rs = np.random.RandomState(1)
    for name, hint in (("exact", areas), ("wrong", rs.permutation(areas)), ("absurd", rs.randint(-5, 2**31 - 1, B).astype(np.int32))):
        for order in (None, True, False):
            SCHED().launch_order = order
            try:
                got = frames_call(la, mix, pf=pf, area_hint=hint)
            finally:
                SCHED().launch_order = None
            for k in ("boxes", "status", "aux"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} hint, launch_order={order}")
    ref = oracle_mix(mix)
    check_strict(want, mix, ref, "B = 300")


# ------------------------------------------------------------------------------------------
# 6. seeded randomised sweep over the campaign generators' shapes
# ------------------------------------------------------------------------------------------
SWEEP_SIZES = [(8, 32), (16, 64), (24, 96), (37, 53), (64, 96), (96, 128), (96, 224), (100, 214), (120, 160), (200, 250), (240, 320), (240, 333),
               (375, 500), (333, 500), (480, 640), (427, 640), (640, 480), (517, 672)]


def sweep_case(rs):
    poly = rs.rand() < 0.3
    P = int(rs.randint(2, 7))
    pool = [s for s in SWEEP_SIZES if not poly or (s[0] <= 240 and s[1] <= 333)]      # (the oracle's rasteriser is a Python loop)
    sizes = [pool[rs.randint(len(pool))] for _ in range(P)]
    depth = [CE.one_plane(rs, h, w) for h, w in sizes]
    skew = rs.rand() < 0.25
    K = np.stack([np.array([[rs.uniform(0.4, 3.0) * w, rs.uniform(-5, 5) if skew else 0.0, w / 2 + rs.uniform(-0.3, 0.3) * w],
                            [0, rs.uniform(0.4, 3.0) * w, h / 2 + rs.uniform(-0.3, 0.3) * h], [0, 0, 1]]) for h, w in sizes])
    masks, segs, img = [], [], []
    for p, (h, w) in enumerate(sizes):
        for _ in range(int(rs.randint(0, 6)) if h * w <= 131072 else int(rs.randint(0, 3))):
            if poly:
                m, seg = CE.one_polygon_mask(rs, h, w)
                segs.append(seg)
            else:
                m = CE.one_mask(rs, h, w)
            masks.append(m); img.append(p)
    if not masks:
        masks.append(np.ones(sizes[0], bool)); img.append(0)
        if poly:
            h, w = sizes[0]
            segs.append([[0.0, 0.0, float(w), 0.0, float(w), float(h), 0.0, float(h)]])
            from oracle import poly_oracle as PO
            masks[0] = PO.create_boolean_mask_from_polygon((w, h), segs[0])[0]
    order = rs.permutation(len(masks))
    mix = dict(sizes=sizes, depth=depth, K=K, masks=[masks[i] for i in order], segs=[segs[i] for i in order] if poly else None,
               img=np.asarray(img, np.int32)[order], expect=None)
    B = len(masks)
    gk = rs.randint(0, 4)
    ground = None
    if gk >= 2:
        ground = np.array([[0.05, -0.97, 0.1, 1.2]] * B) + 0.05 * rs.randn(B, 4)
        if gk == 3:
            for n in range(B):
                r = rs.rand()
                if r < 0.25:
                    ground[n, 0] = np.nan
                elif r < 0.32:
                    ground[n] = [0, -1, 0, 1.0]          # the reference's degenerate case (status 2)
    sidx = draws(mix, int(rs.randint(1 << 30))) if rs.rand() < 0.25 else None
    return mix, ground, sidx


@pytest.mark.parametrize("chunk", range(4))
def test_randomised_sweep(la, chunk):
    """4 x 26 = 104 seeded cases, none skipped, no instance waived: random size mixes, the campaign generators' mask shapes and depth
    planes (invalid pixels included), polygons, ground rows, skewed cameras, subsample mode - against the oracle by the campaign's
    rule (see the module docstring), and status / n_in / n_valid (of the fitted) against the uniform entry run size group by size group"""
    rs = np.random.RandomState(7000 + chunk)
    n_ok = n_all = n_tie = 0
    for case in range(26):
        mix, ground, sidx = sweep_case(rs)
        B = len(mix["masks"])
        tag = f"chunk {chunk} case {case}: B={B} sizes={mix['sizes']} poly={mix['segs'] is not None} ground={ground is not None} sample={sidx is not None}"
        rec, st, yaw, nv, kap = oracle_mix(mix, ground, sidx, kappa=True)
        got = frames_call(la, mix, ground=ground, sample_idx=sidx)
        np.testing.assert_array_equal(got["status"], st, err_msg=tag + " status")
        ok = st == 0
        assert np.isnan(got["boxes"][~ok]).all(), tag
        np.testing.assert_array_equal(got["aux"][:, 2], [m.sum() for m in mix["masks"]], err_msg=tag + " n_in")
        np.testing.assert_array_equal(got["aux"][ok, 1], nv[ok], err_msg=tag + " n_valid")
        tie = ok & ~(got["aux"][:, 3] >= 1e-9)
        chk = ok & ~tie
        noise = reference_axis_noise(kap, got["aux"][:, 1], got["aux"][:, 3])
        assert_records(got["boxes"][chk], rec[chk], tag, gap=got["aux"][chk, 3], noise=noise[chk])
        want = grouped_call(la, mix, ground=ground, sample_idx=sidx)
        np.testing.assert_array_equal(got["status"], want["status"], err_msg=tag + " vs uniform entry")
        # (n_valid of a REJECTED instance is whatever the engine had counted when it gave up: small grounded batches of the uniform entry
        # run on another engine)
        np.testing.assert_array_equal(got["aux"][:, 2], want["aux"][:, 2], err_msg=tag + " vs uniform entry")
        np.testing.assert_array_equal(got["aux"][ok, 1], want["aux"][ok, 1], err_msg=tag + " vs uniform entry")
        n_ok += int(chk.sum()); n_all += B; n_tie += int(tie.sum())
    print(f"sweep chunk {chunk}: {n_ok} of {n_all} instances compared record by record ({n_tie} exact ties)")
    assert 3 * n_ok >= n_all


# ------------------------------------------------------------------------------------------
# 7. the scene pipeline
# ------------------------------------------------------------------------------------------
def _scenes_of_four_sizes(with_ground=False):
    from labelany3d_amd.fit_scenes import synthetic_scenes

    per = []
    for k, (h, w) in enumerate([(480, 640), (427, 640), (375, 500), (500, 333)]):
        sc, _ = synthetic_scenes(6, seed=100 + k, H=h, W=w, with_ground=with_ground)
        for s in sc:
            s["name"] = f"{h}x{w}-" + s["name"]
        per.append(sc)
    return [s for group in zip(*per) for s in group]        # interleaved: every batch of the mixed mode holds all four sizes


def _run_pipeline(scenes, **kw):
    from labelany3d_amd.fit_scenes import ScenePipeline

    pipe = ScenePipeline(batch_images=8, write=False, **kw)
    return {sc["name"]: recs.text for sc, recs in pipe.run(scenes)}


def test_pipeline_mixed_frames_writes_the_same_files(la):
    scenes = _scenes_of_four_sizes()
    default = _run_pipeline(scenes)
    mixed = _run_pipeline(scenes, mixed_frames=True)
    assert sorted(default) == sorted(mixed) == sorted(sc["name"] for sc in scenes) and len(default) == 24
    n_boxes = 0
    for name in default:
        assert mixed[name] == default[name], f"{name}: 3dbbox.json differs between the mixed and the default mode"
        n_boxes += len(json.loads(default[name]))
    assert n_boxes >= 48
    with pytest.raises(ValueError, match="pca"):
        _run_pipeline(scenes, mixed_frames=True, method="convex_hull")


def test_pipeline_mixed_frames_two_phase(la):
    """ground files make the pipeline take its two-phase form (statistics pass, then the fit with per-instance ground rows): the same
    scenes, the same objects; the default mode fits its small grounded batches on another engine, so the numbers agree to 1e-9"""
    scenes = _scenes_of_four_sizes(with_ground=True)
    default = _run_pipeline(scenes)
    mixed = _run_pipeline(scenes, mixed_frames=True)
    n = 0
    for name in default:
        a, b = json.loads(default[name]), json.loads(mixed[name])
        assert [(r["obj_id"], r["category_name"]) for r in a] == [(r["obj_id"], r["category_name"]) for r in b], name
        for ra, rb in zip(a, b):
            for key in ("center_cam", "dimensions", "R_cam", "bbox3D_cam"):
                np.testing.assert_allclose(np.asarray(rb[key], float), np.asarray(ra[key], float), rtol=1e-9, atol=1e-9, err_msg=f"{name} {key}")
            n += 1
    assert n >= 48
    sub = _run_pipeline(scenes, mixed_frames=True, subsample=True, rng=np.random.RandomState(5))
    assert sorted(sub) == sorted(default) and sum(len(json.loads(t)) for t in sub.values()) == n
