"""GPU tests of the convex-hull yaw for the depth + mask fit (``method="convex_hull"``, la3d_fit_args::method) against
``oracle.fit_instances(method="convex_hull")``.

Comparison rule for hull records, taken from the project: ``tests/test_gpu_parity.py::assert_records`` (rtol 1e-9); where that
fails, the two waivers of ``oracle/campaigns/points.py::check_run`` and no other - the two footprint areas agree within 1e-9
relative (a tied minimum), or both are below 1e-9 x extent^2 (a flat footprint) - and the height (dims[1], center y) must agree
regardless.  Waived instances are at most 5 % of any test's instances (asserted).  The inputs keep the oracle alone far inside
that cap: per-pixel Gaussian depth noise, elliptic masks (tests/test_hull_contract.py checks the same scenes oracle against oracle).
The small frames are 224 x 96: the tiled path of the instance engine, which the full-mask hull rests on, wants at least 64 tiles of
32 x 8 pixels."""
import ctypes as C

import numpy as np
import pytest

from oracle import la3d_oracle as O
from oracle.campaigns.points import footprint_area

from .conftest import SCHED
from .test_gpu_parity import assert_records, np_
from .test_hull_contract import hull_scene as _hull_scene

pytestmark = pytest.mark.gpu


def hull_scene(*a, **k):
    """tests/test_hull_contract.py's scenes with masks that leave room for the column arrays behind their tile list on the small
    frames too (full-mask hull: active tiles x 32 B + 8 W bytes within the bit image's H W / 8 bytes - 28 of the 84 tiles of a
    224 x 96 frame, 904 of the 1200 of a 640 x 480 one, where the tile list is the limit; larger masks are refused, test_full_mask_refuses_...)"""
    k.setdefault("rmax", 0.2)
    return _hull_scene(*a, **k)


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def assert_hull_records(got, ref, tag, cap=0.05):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    waived = 0
    for n in range(len(ref)):
        try:
            assert_records(got[n:n + 1], ref[n:n + 1], f"{tag}[{n}]")
        except AssertionError:
            if np.isnan(ref[n]).all() or np.isnan(got[n]).any():
                raise
            ext = max(np.abs(ref[n, 3:6]).max(), 1e-300)
            fg, fr = footprint_area(got[n]), footprint_area(ref[n])
            height = abs(got[n, 4] - ref[n, 4]) <= 1e-9 * max(ext, 1.0) and abs(got[n, 1] - ref[n, 1]) <= 1e-9 * max(ext, abs(ref[n, 1]), 1.0)
            tied = abs(fg - fr) <= 1e-9 * max(fr, 1e-300)
            flat = max(fg, fr) <= 1e-9 * ext * ext
            if not (height and (tied or flat)):
                raise
            waived += 1
    print(f"{tag}: {waived} of {len(ref)} records waived (tied / flat footprint)")
    assert waived <= cap * len(ref), f"{tag}: {waived} of {len(ref)} records needed a waiver"


def check_against_oracle(got, depth, masks, K, tag, ground=None, sample_idx=None, depth_index=None, hull_decided=True):
    boxes, status, aux = (np_(t) for t in got)
    ref, st, yaw, nv = O.fit_instances(depth, masks, K, ground=ground, sample_idx=sample_idx, depth_index=depth_index, method="convex_hull")
    if ground is not None:   # a row whose first entry is NaN means "no ground" for that instance (la3d.h): the oracle is told None there
        r0, s0, _, n0 = O.fit_instances(depth, masks, K, ground=None, sample_idx=sample_idx, depth_index=depth_index, method="convex_hull")
        free = np.isnan(np.asarray(ground)[:, 0])
        ref[free], st[free], nv[free] = r0[free], s0[free], n0[free]
    np.testing.assert_array_equal(status, st, err_msg=tag)
    ok = st == 0
    assert np.isnan(boxes[~ok]).all(), tag
    np.testing.assert_array_equal(aux[ok, 1], nv[ok], err_msg=tag)
    np.testing.assert_array_equal(aux[:, 2], masks.reshape(len(masks), -1).sum(1), err_msg=tag)
    if hull_decided:
        assert (aux[ok, 3] <= -3).all(), (tag, aux[ok, 3].max())
    assert_hull_records(boxes, ref, tag)
    return boxes, status, aux, ref


def ellipse_polygons(seed, B, H, W):
    rs = np.random.RandomState(seed)
    segs = []
    for _ in range(B):
        cy, cx = rs.uniform(0.25, 0.75) * H, rs.uniform(0.25, 0.75) * W
        ry, rx = rs.uniform(0.08, 0.24) * H, rs.uniform(0.08, 0.24) * W
        t = np.linspace(0, 2 * np.pi, 24, endpoint=False)
        segs.append([np.stack([cx + rx * np.cos(t), cy + ry * np.sin(t)], 1).reshape(-1).tolist()])
    return segs


def same_masks_three_ways(la, seed, B, H, W):
    """polygon parts, the u8 planes they rasterise to, and the run lengths of those planes; depth as hull_scene"""
    depth, _, K = hull_scene(seed, B, H, W)
    polys = la.pack_polygons(ellipse_polygons(seed + 1, B, H, W), H, W)
    masks = np_(la.poly_decode(polys)).astype(bool)
    rles = [O.rle_encode(m) for m in masks]
    return depth, masks, rles, polys, K


# ------------------------------------------------------------------------------------------
# full-mask mode, no ground
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(7, 96, 224), (300, 96, 224), (1100, 96, 224), (64, 480, 640)])
def test_full_mask_three_sources(la, B, H, W):
    """u8, run-length and polygon input of the same masks; B below, across and above the batch limits of the other engines (160)
    and of the launch-order range (256)"""
    depth, masks, rles, polys, K = same_masks_three_ways(la, 100 + B, B, H, W)
    got = la.fit_instances(depth, masks, K, method="convex_hull")
    check_against_oracle(got, depth, masks, K, f"u8 B={B} {W}x{H}")
    for name, other in (("rle", la.fit_instances_rle(depth, rles, K, method="convex_hull")),
                        ("poly", la.fit_instances_poly(depth, polys, K, method="convex_hull"))):
        for a, b in zip(got, other):
            np.testing.assert_array_equal(np_(a), np_(b), err_msg=f"{name} input differs from u8 input")


def test_height_not_a_multiple_of_8_and_padded_width(la):
    depth, masks, K = hull_scene(7, 12, 100, 224)
    check_against_oracle(la.fit_instances(depth, masks, K, method="convex_hull"), depth, masks, K, "H=100")
    # a frame 214 columns wide: run lengths, the wrapper pads the depth rows to 224 and says frame_width = 214
    depth, masks, K = hull_scene(8, 12, 96, 214)
    rles = [O.rle_encode(m) for m in masks]
    check_against_oracle(la.fit_instances_rle(depth, rles, K, method="convex_hull"), depth, masks, K, "W=214 rle")
    # u8 planes of that frame: the wrapper pads planes and rows
    check_against_oracle(la.fit_instances(depth, masks, K, method="convex_hull"), depth, masks, K, "W=214 u8")


def test_image_index_shared_planes_and_proj(la):
    from labelany3d_amd.masks import fit_instances_ex

    B, P, H, W = 20, 3, 96, 224
    depth, masks, K = hull_scene(9, B, H, W, nan_every=0)
    depth = depth[:P]
    Ks = np.stack([K, K * [[1.1], [0.9], [1]], K * [[0.9], [1.2], [1]]])
    ii = (np.arange(B) % P).astype(np.int32)
    r = fit_instances_ex(depth, Ks, masks=masks, image_index=ii, image_size=(W, H), method="convex_hull")
    boxes, _, _, ref = check_against_oracle((r["boxes"], r["status"], r["aux"]), depth, masks, Ks, "image_index", depth_index=ii)
    for n in range(B):
        want = O.project_boxes(boxes[n:n + 1], Ks[ii[n]], (W, H))
        np.testing.assert_allclose(np_(r["boxes2d"])[n], np.ravel(want), rtol=1e-9, atol=1e-9)


def test_fused_filter_keeps_status_6_rows_nan(la):
    B, H, W = 24, 96, 224
    depth, _, K = hull_scene(10, B, H, W)
    masks = np_(la.poly_decode(la.pack_polygons(ellipse_polygons(11, B, H, W), H, W))).astype(bool)   # (clear of the border strips)
    masks[3] = False; masks[3, 40:44, 50:54] = True        # below min_area
    masks[5] = False; masks[5, 0:60, 0:40] = True          # touches the border
    rles = [O.rle_encode(m) for m in masks]
    fb, fs, fa, stats = la.fit_instances_rle(depth, rles, K, filter=True, method="convex_hull")
    ub, us, ua = la.fit_instances_rle(depth, rles, K, method="convex_hull")
    fs = np_(fs)
    assert fs[3] == 6 and fs[5] == 6 and (fs != 6).sum() >= B // 2
    assert np.isnan(np_(fb)[fs == 6]).all()
    keep = fs != 6
    np.testing.assert_array_equal(np_(fb)[keep], np_(ub)[keep])
    np.testing.assert_array_equal(fs[keep], np_(us)[keep])
    check_against_oracle((ub, us, ua), depth, masks, K, "rle unfiltered")


# ------------------------------------------------------------------------------------------
# NaN holes, all-NaN, inf, negative depth; the collinear fallback
# ------------------------------------------------------------------------------------------
def test_nonfinite_and_negative_depths_under_the_mask(la):
    B, H, W = 10, 96, 224
    depth, masks, K = hull_scene(11, B, H, W, nan_every=2, negative_at=3)
    depth[4][masks[4]] = np.nan                                   # all NaN: status 1
    r, c = np.argwhere(masks[5])[10]
    depth[5, r, c] = np.inf                                       # an inf: dropped like a NaN
    r, c = np.argwhere(masks[6])[20]
    depth[6, r, c] = -np.inf
    got = la.fit_instances(depth, masks, K, method="convex_hull")
    boxes, status, aux, _ = check_against_oracle(got, depth, masks, K, "nonfinite")
    assert status[4] == 1 and status[5] == 0 and status[6] == 0 and status[3] == 0
    _, ps, pa = la.fit_instances(depth, masks, K)                 # the PCA call of the same instances
    np.testing.assert_array_equal(status, np_(ps))
    np.testing.assert_array_equal(aux[:, 1], np_(pa)[:, 1])
    assert aux[5, 1] == masks[5].sum() - (~np.isfinite(depth[5][masks[5]])).sum()


def test_constant_depth_takes_the_pca_fallback(la):
    B, H, W = 6, 96, 224
    depth, masks, K = hull_scene(12, B, H, W, nan_every=0)
    depth[1][:] = 3.25                                            # exactly collinear footprint: equal z, every turn test an exact zero
    depth[4][:] = 1.5
    got = la.fit_instances(depth, masks, K, method="convex_hull")
    boxes, status, aux, ref = check_against_oracle(got, depth, masks, K, "constant depth", hull_decided=False)
    assert (status == 0).all()
    assert aux[1, 3] >= 0 and aux[4, 3] >= 0
    assert (aux[[0, 2, 3, 5], 3] <= -3).all()
    pb, _, _ = la.fit_instances(depth, masks, K)
    assert_records(boxes[[1, 4]], ref[[1, 4]], "fallback vs oracle")
    assert_records(boxes[[1, 4]], np_(pb)[[1, 4]], "fallback vs the PCA call")


# ------------------------------------------------------------------------------------------
# reference-subsample mode: every camera, every ground vector
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["no_ground", "ground", "skewed_K"])
def test_subsample_mode(la, case):
    B, H, W = 40, 96, 224
    depth, masks, K = hull_scene(13, B, H, W)
    for n in (2, 9):                                              # masks of at most 500 pixels: not sampled
        masks[n] = False
        masks[n, 30:30 + 12 + n, 40:60] = True
    ground = None
    if case == "ground":
        rs = np.random.RandomState(3)
        ground = np.array([[0.02, -0.98, 0.1, 1.5]] * B) + 0.03 * rs.randn(B, 4)
        ground[::4, 0] = np.nan
    if case == "skewed_K":
        K = K.copy()
        K[0, 1] = 3.0
    counts = masks.reshape(B, -1).sum(1)
    assert (counts[[2, 9]] <= 500).all() and (counts > 500).sum() > 20
    sidx = la.draw_sample_idx(counts, np.random.RandomState(17))
    got = la.fit_instances(depth, masks, K, ground=ground, sample_idx=sidx, method="convex_hull")
    check_against_oracle(got, depth, masks, K, case, ground=ground, sample_idx=sidx)
    rles = [O.rle_encode(m) for m in masks]
    other = la.fit_instances_rle(depth, rles, K, ground=ground, sample_idx=sidx, method="convex_hull")
    for a, b in zip(got, other):
        np.testing.assert_array_equal(np_(a), np_(b))


# ------------------------------------------------------------------------------------------
# refusals, pins, the argument block, graphs
# ------------------------------------------------------------------------------------------
def test_full_mask_refuses_ground_rows_and_skewed_K(la):
    B, H, W = 16, 96, 224
    depth, masks, K = hull_scene(14, B, H, W)
    ground = np.full((B, 4), np.nan)
    grounded = np.zeros(B, bool)
    grounded[[1, 6, 7, 13]] = True
    ground[grounded] = [0.02, -0.98, 0.1, 1.5]
    masks[10] = True                                              # a mask whose tile list leaves no room for the column arrays
    grounded[10] = True                                           # (refused like the grounded ones)
    boxes, status, aux = (np_(t) for t in la.fit_instances(depth, masks, K, ground=ground, method="convex_hull"))
    ref, st, _, _ = O.fit_instances(depth, masks, K, method="convex_hull")
    np.testing.assert_array_equal(status, np.where(grounded, 5, st))
    assert np.isnan(boxes[grounded]).all()
    assert_hull_records(boxes[~grounded], ref[~grounded], "beside refused instances")
    # a skewed K on some images
    Ks = np.stack([K] * B)
    skew = np.zeros(B, bool)
    skew[[0, 5, 10, 11]] = True                                   # (10: the whole-frame mask, refused either way)
    Ks[skew, 0, 1] = 2.0
    boxes, status, aux = (np_(t) for t in la.fit_instances(depth, masks, Ks, method="convex_hull"))
    np.testing.assert_array_equal(status, np.where(skew, 5, st))
    assert np.isnan(boxes[skew]).all()
    assert_hull_records(boxes[~skew], ref[~skew], "beside skewed cameras")


@pytest.mark.parametrize("engine", ["rows", "band", "split"])
def test_pinned_engines_give_way(la, engine, monkeypatch):
    depth, masks, K = hull_scene(15, 12, 96, 224)
    want = [np_(t) for t in la.fit_instances(depth, masks, K, method="convex_hull")]
    monkeypatch.setattr(SCHED(), "engine", engine)
    monkeypatch.setattr(SCHED(), "build", "plain")                # a speed option that switches the single pass off: ignored too
    got = [np_(t) for t in la.fit_instances(depth, masks, K, method="convex_hull")]
    for a, b in zip(want, got):
        np.testing.assert_array_equal(a, b)
    assert (got[1] == 0).all() and (got[2][:, 3] <= -3).all()


def test_old_struct_size_and_method_0_equal_the_positional_entry(la):
    import torch

    from labelany3d_amd._lib import FitArgs, lib

    depth, masks, K = hull_scene(16, 9, 96, 224)
    B, H, W = masks.shape
    dev = torch.device("cuda", 0)
    d = torch.as_tensor(depth, device=dev)
    m = torch.as_tensor(masks.view(np.uint8), device=dev)
    k = torch.as_tensor(K[None], device=dev)
    ws = torch.empty(lib.la3d_workspace_bytes(B, H, W) + 256, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def outputs():
        return (torch.full((B, 39), 7.0, dtype=torch.float64, device=dev), torch.full((B,), -1, dtype=torch.int32, device=dev),
                torch.full((B, 4), 7.0, dtype=torch.float64, device=dev))
    o0 = outputs()
    assert lib.la3d_fit_instances(p(d), H * W, None, p(m), p(k), 0, None, None, B, H, W, p(o0[0]), p(o0[1]), p(o0[2]), p(ws), None) == 0
    torch.cuda.synchronize()
    # (a block cut off in front of `method` - whatever bytes follow it in the caller's memory - and a block that says 0)
    for size, method in ((FitArgs.method.offset, 1), (C.sizeof(FitArgs), 0)):
        o = outputs()
        a = FitArgs(struct_size=size, B=B, H=H, W=W, depth=p(d), depth_plane_stride=H * W, mask=p(m), K=p(k), out=p(o[0]), status=p(o[1]),
                    aux=p(o[2]), workspace=p(ws), method=method)
        assert lib.la3d_fit_instances_ex(C.byref(a)) == 0
        torch.cuda.synchronize()
        for x, y in zip(o0, o):
            assert torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)), (size, method)
    assert (np_(o0[2])[:, 3] >= 0).all()   # PCA records: the eigen-gap


def test_hull_call_captured_into_a_graph(la):
    """the two launches of a hull call are one linear chain on one stream: captured once, replayed on fresh inputs"""
    import torch

    from labelany3d_amd import InstanceFitter

    B, H, W = 48, 96, 224
    dev = torch.device("cuda", 0)
    depth0, masks0, K = hull_scene(17, B, H, W)
    d = torch.as_tensor(depth0, device=dev)
    m = torch.as_tensor(masks0.view(np.uint8), device=dev)
    k = torch.as_tensor(K, device=dev)
    f = InstanceFitter(B, H, W, dev, method="convex_hull")
    side = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        f.run(d, m, k, stream=side)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            f.run(d, m, k, stream=torch.cuda.current_stream())
    fr = InstanceFitter(B, H, W, dev, method="convex_hull")
    for seed in (18, 19):
        depth1, masks1, _ = hull_scene(seed, B, H, W)
        d.copy_(torch.as_tensor(depth1, device=dev)); m.copy_(torch.as_tensor(masks1.view(np.uint8), device=dev))
        f.boxes.fill_(12345.0); f.status.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        rb, rs_, ra = fr.run(d, m, k)
        torch.cuda.synchronize()
        assert torch.equal(f.status[0], rs_) and (rs_ == 0).all()
        assert torch.equal(f.boxes[0], rb) and torch.equal(f.aux[0], ra)
    # and a fitter sized for PCA refuses a hull call instead of overrunning its workspace
    with pytest.raises(ValueError, match="sized for method='pca'"):
        InstanceFitter(B, H, W, dev).run(d, m, k, method="convex_hull")


# ------------------------------------------------------------------------------------------
# annotations and scenes
# ------------------------------------------------------------------------------------------
def test_fit_annotations_and_scene_pipeline(la):
    import torch

    from labelany3d_amd import fit_scenes as F
    from labelany3d_amd.masks import fit_annotations, fit_annotations_all, segmentations_to_masks

    scenes, _ = F.synthetic_scenes(6, seed=31, H=192, W=256, mean_instances=6.0, rle_fraction=0.4)
    piped = {sc["name"]: recs for sc, recs in F.ScenePipeline(batch_images=4, write=False, method="convex_hull").run(scenes)}
    n_boxes = 0
    for sc in scenes:
        H, W, K = sc["height"], sc["width"], np.asarray(sc["K"], dtype=np.float64)
        anns = sc["annotations"]
        _, kept, _, boxes, status = fit_annotations(anns, (W, H), sc["depth"], K, method="convex_hull")
        d_dev = torch.as_tensor(sc["depth"], device="cuda")
        _, kept_h, _, boxes_h, status_h = fit_annotations(anns, (W, H), d_dev, K, to_host=True, method="convex_hull")   # the la3d_fit_annotations_host route
        np.testing.assert_array_equal(kept, kept_h)
        np.testing.assert_array_equal(np_(boxes), boxes_h)
        ab, as_ = fit_annotations_all(anns, (W, H), sc["depth"], K, filter=True, method="convex_hull")
        np.testing.assert_array_equal(np_(ab)[kept], np_(boxes))
        # the fit_instances hull records of the same masks
        masks = segmentations_to_masks([anns[i]["segmentation"] for i in kept], H, W)
        ib, ist, _ = la.fit_instances(sc["depth"], masks, K, method="convex_hull")
        np.testing.assert_array_equal(np_(status), np_(ist))
        np.testing.assert_array_equal(np_(boxes), np_(ib))
        ok = np_(status) == 0
        got = piped[sc["name"]]
        assert len(got) == ok.sum()
        for g, rec in zip(got, np_(boxes)[ok]):
            flat = np.concatenate([g["center_cam"], g["dimensions"], np.ravel(g["R_cam"]), np.ravel(g["bbox3D_cam"])])
            np.testing.assert_array_equal(flat, rec)
        n_boxes += int(ok.sum())
    assert n_boxes >= 10
