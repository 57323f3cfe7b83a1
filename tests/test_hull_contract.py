"""CPU-only contract of the convex-hull yaw for the depth + mask fit (la3d_fit_args::method): the argument block and the size
function, the ``method`` keyword of every Python entry (rejected before any device work with the reference's message,
src/util_3dbox.py:151), and the column-end claim the full-mask hull rests on, checked oracle against oracle."""
import ctypes as C
import inspect

import numpy as np
import pytest

from oracle import la3d_oracle as O

MSG = r"Unknown method: obb\. Use 'pca' or 'convex_hull'"


def test_fit_args_ends_in_method_and_size_function():
    from labelany3d_amd import _lib

    assert _lib.FitArgs._fields_[-1][0] == "method"
    assert "la3d_fit_workspace_bytes" in _lib.EXPORTS
    for B, H, W in ((1, 480, 640), (64, 480, 640), (1024, 480, 640), (7, 37, 53), (300, 96, 160)):
        base = _lib.lib.la3d_workspace_bytes(B, H, W)
        assert _lib.fit_workspace_bytes(B, H, W, _lib.METHOD_PCA) == base
        hull = _lib.fit_workspace_bytes(B, H, W, _lib.METHOD_CONVEX_HULL)
        # per instance at least the larger hand-off: 2 W column words, or 500 points of three doubles
        assert hull >= base + B * max(2 * W * 4, 500 * 24)
    assert _lib.fit_workspace_bytes(0, 480, 640, _lib.METHOD_CONVEX_HULL) == 0
    # a block of the size published before the field existed means PCA
    a = _lib.FitArgs(struct_size=_lib.FitArgs.method.offset, B=64, H=480, W=640, method=_lib.METHOD_CONVEX_HULL)
    assert _lib.lib.la3d_fit_workspace_bytes(C.byref(a)) == _lib.lib.la3d_workspace_bytes(64, 480, 640)


def test_unknown_method_is_an_argument_error_without_a_device():
    """la3d_fit_instances_ex checks the block before it launches anything: no GPU is needed to be refused."""
    from labelany3d_amd import _lib

    one = (C.c_double * 64)()
    a = _lib.FitArgs(struct_size=C.sizeof(_lib.FitArgs), B=1, H=8, W=32, depth=C.addressof(one), mask=C.addressof(one),
                     K=C.addressof(one), out=C.addressof(one), status=C.addressof(one), workspace=C.addressof(one), method=2)
    assert _lib.lib.la3d_fit_instances_ex(C.byref(a)) == -1
    assert b"method" in _lib.lib.la3d_last_error()


def _entries():
    import labelany3d_amd as la
    from labelany3d_amd import batched, fit_scenes, masks, pipeline, shard

    d, m, K = np.zeros((8, 32), np.float32), np.zeros((1, 8, 32), bool), np.eye(3)
    rle = [{"size": [8, 32], "counts": [0, 8, 248]}]
    poly = masks.pack_polygons([[[1, 1, 9, 1, 9, 6]]], 8, 32)
    ann = [{"segmentation": [[1, 1, 9, 1, 9, 6]], "bbox": [1, 1, 8, 5], "category_id": 1}]
    return {
        "fit_instances": (la.fit_instances, lambda f: f(d, m, K, method="obb")),
        "InstanceFitter.run": (batched.InstanceFitter.run, lambda f: batched.InstanceFitter(1, 8, 32, method="obb")),
        "masks.fit_instances_ex": (masks.fit_instances_ex, lambda f: f(d, K, masks=m, method="obb")),
        "fit_instances_rle": (masks.fit_instances_rle, lambda f: f(d, rle, K, method="obb")),
        "fit_instances_poly": (masks.fit_instances_poly, lambda f: f(d, poly, K, method="obb")),
        "fit_annotations": (masks.fit_annotations, lambda f: f(ann, (32, 8), d, K, method="obb")),
        "fit_annotations_all": (masks.fit_annotations_all, lambda f: f(ann, (32, 8), d, K, method="obb")),
        "fit_instances_sharded": (shard.fit_instances_sharded, lambda f: f(d[None], m, K, [0], method="obb")),
        "fit_annotations_sharded": (shard.fit_annotations_sharded, lambda f: f(ann, (32, 8), [0], 1, None, method="obb")),
        "pipeline.fit_batches": (pipeline.fit_batches, lambda f: next(f([(d, m, K)], method="obb"))),
        "ScenePipeline": (fit_scenes.ScenePipeline.__init__, lambda f: fit_scenes.ScenePipeline(method="obb")),
    }


@pytest.mark.parametrize("name", ["fit_instances", "InstanceFitter.run", "masks.fit_instances_ex", "fit_instances_rle", "fit_instances_poly",
                                  "fit_annotations", "fit_annotations_all", "fit_instances_sharded", "fit_annotations_sharded",
                                  "pipeline.fit_batches", "ScenePipeline"])
def test_every_entry_has_the_keyword_and_rejects_unknown_methods_first(name, monkeypatch):
    import torch

    # "before touching a device": any attempt to look for one fails the test
    def no_device(*a, **k):
        raise AssertionError("the entry touched the device before it checked `method`")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    fn, call = _entries()[name]
    par = inspect.signature(fn).parameters["method"]
    assert par.default in ("pca", None)   # (InstanceFitter.run: None = what the fitter was built for, "pca" by default)
    with pytest.raises(ValueError, match=MSG):
        call(fn)


def test_fitter_default_method_is_pca():
    from labelany3d_amd import batched

    assert inspect.signature(batched.InstanceFitter.__init__).parameters["method"].default == "pca"


def test_fit_scenes_bbox_method_parses():
    from labelany3d_amd import fit_scenes

    ap = fit_scenes.build_parser()
    assert ap.parse_args(["--scenes", "x"]).bbox_method == "pca"
    assert ap.parse_args(["--scenes", "x", "--bbox-method", "convex_hull"]).bbox_method == "convex_hull"
    with pytest.raises(SystemExit):
        ap.parse_args(["--scenes", "x", "--bbox-method", "obb"])


# ------------------------------------------------------------------------------------------
# the column-end claim: without ground rotation and skew all points of pixel column u lie on one ray through the origin of
# the x/z plane, so the hull of a mask is the hull of each column's nearest and farthest valid point
# ------------------------------------------------------------------------------------------
def hull_scene(seed, B, H, W, nan_every=5, negative_at=None, rmax=0.3):
    """B elliptic masks on a noisy sloped depth plane (0.05 m Gaussian noise: no tied minimum-area edges), NaN holes in every
    ``nan_every``-th instance's own plane, one negative depth under instance ``negative_at``; half axes up to ``rmax`` of the frame."""
    rs = np.random.RandomState(seed)
    vv, uu = np.mgrid[0:H, 0:W]
    depth = np.empty((B, H, W), np.float32)
    masks = np.zeros((B, H, W), bool)
    for n in range(B):
        depth[n] = (2.0 + rs.uniform(0, 3) + rs.uniform(-0.004, 0.004) * uu + rs.uniform(-0.003, 0.003) * vv
                    + 0.05 * rs.randn(H, W)).astype(np.float32)
        cy, cx = rs.uniform(0.2, 0.8) * H, rs.uniform(0.2, 0.8) * W
        ry, rx = rs.uniform(0.08, rmax) * H, rs.uniform(0.08, rmax) * W
        masks[n] = ((vv - cy) / ry) ** 2 + ((uu - cx) / rx) ** 2 <= 1.0
        if nan_every and n % nan_every == 0:
            holes = masks[n] & (rs.rand(H, W) < 0.05)
            depth[n][holes] = np.nan
        if negative_at is not None and n == negative_at:
            r, c = np.argwhere(masks[n] & np.isfinite(depth[n]))[3]
            depth[n, r, c] = -1.5
    K = np.array([[0.8 * W, 0, W / 2.0], [0, 0.8 * W, H / 2.0], [0, 0, 1]])
    return depth, masks, K


def column_end_candidates(pts_hw3, mask, depth):
    """Per occupied pixel column the points of the smallest and the largest valid depth."""
    out = []
    for u in np.flatnonzero(mask.any(axis=0)):
        rows = np.flatnonzero(mask[:, u] & np.isfinite(depth[:, u]))
        if len(rows):
            d = depth[rows, u]
            out += [pts_hw3[rows[np.argmin(d)], u], pts_hw3[rows[np.argmax(d)], u]]
    return np.asarray(out).reshape(-1, 3)


def test_column_end_candidates_give_the_hull_yaw_of_all_points():
    B, H, W = 64, 96, 160
    depth, masks, K = hull_scene(20261016, B, H, W, negative_at=7)
    worst, most = 0.0, 0
    for n in range(B):
        pts = O.depth_to_points(depth[n][None], K)
        cloud = pts[masks[n]]
        cloud = cloud[~np.isnan(cloud).any(axis=1)]
        cand = column_end_candidates(pts, masks[n], depth[n])
        assert 3 <= len(cand) <= 2 * W
        most = max(most, len(cand))
        y_all, y_cand = O.yaw_convex_hull(cloud), O.yaw_convex_hull(cand)
        worst = max(worst, abs(y_all - y_cand))
        # and the extents under that yaw are taken at candidates (every hull vertex is one)
        r_all, r_cand = O.rotate_y(y_all) @ cloud.T, O.rotate_y(y_all) @ cand.T
        np.testing.assert_allclose(r_cand[[0, 2]].min(axis=1), r_all[[0, 2]].min(axis=1), rtol=0, atol=1e-12)
        np.testing.assert_allclose(r_cand[[0, 2]].max(axis=1), r_all[[0, 2]].max(axis=1), rtol=0, atol=1e-12)
    assert worst < 1e-9, worst
    assert most <= 2 * W
