"""GPU test of ``ScenePipeline(export_points=True)``: a synthetic tree of six scenes of three sizes (one of odd width), in both
pipeline modes and with uint16 depth - ``3dbbox.json`` byte-identical to the run without the flag, exactly one PLY per record and none
for dropped instances, the vertices the float32 cast of the oracle's cloud of the full mask with the non-finite rows removed."""
import json
import os

import numpy as np
import pytest

from oracle import la3d_oracle as O
from oracle import poly_oracle as P

from .test_ply_contract import read_ply

pytestmark = pytest.mark.gpu

SIZES = ((240, 320), (200, 333), (192, 256))   # (H, W): 333 is padded to 352 on the device
SCALE = 0.001


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


_SCENES = {}


def scenes_of(depth_dtype):
    """two scenes per size, interleaved so that a mixed batch meets the sizes in turn (computed once per dtype, never written to)"""
    from labelany3d_amd import fit_scenes as FS

    if depth_dtype not in _SCENES:
        per_size = [FS.synthetic_scenes(2, seed=7 + s, H=h, W=w, mean_instances=14.0, rle_fraction=0.4, depth_dtype=depth_dtype,
                                        depth_scale=SCALE)[0] for s, (h, w) in enumerate(SIZES)]
        scenes = []
        for i in range(2):
            for s, group in enumerate(per_size):
                sc = dict(group[i])
                sc["name"] = f"size{s}_{sc['name']}"
                scenes.append(sc)
        _SCENES[depth_dtype] = scenes
    return _SCENES[depth_dtype]


def run_tree(root, scenes, **kw):
    from labelany3d_amd import fit_scenes as FS

    placed = []
    for sc in scenes:
        d = os.path.join(str(root), sc["name"])
        os.makedirs(d)
        placed.append(dict(sc, dir=d))
    pipe = FS.ScenePipeline(batch_images=4, write=True, **kw)
    done = {sc["name"]: recs for sc, recs in pipe.run(placed)}
    assert len(done) == len(scenes)
    return placed


def kept_masks(sc):
    """the reference's reader on the CPU oracle: the masks of the kept instances of a scene, in annotation order (index = obj_id)"""
    H, W = sc["height"], sc["width"]
    kept = []
    for a in sc["annotations"]:
        seg = a.get("segmentation")
        if a.get("iscrowd") or not seg:
            continue
        rle = isinstance(seg, dict)
        m = O.rle_decode(seg["counts"], H, W) if rle else P.create_boolean_mask_from_polygon((W, H), seg)[0]
        if O.keep_instance(O.mask_stats(m, 10), H, rle):
            kept.append(m)
    return kept


@pytest.mark.parametrize("mixed", [False, True], ids=["by size", "mixed frames"])
@pytest.mark.parametrize("depth_dtype", [None, "u16"], ids=["f32", "u16"])
def test_one_ply_per_record(la, tmp_path, mixed, depth_dtype):
    scenes = scenes_of(depth_dtype)
    kw = dict(mixed_frames=mixed, depth_dtype=depth_dtype, depth_scale=SCALE)
    plain = run_tree(tmp_path / "plain", scenes, **kw)
    flagged = run_tree(tmp_path / "flagged", scenes, export_points=True, **kw)
    assert check_trees(plain, flagged, depth_dtype) >= 12


def check_trees(plain, flagged, depth_dtype=None):
    """the three properties of the export, scene by scene -> the number of records"""
    total = 0
    for a, b in zip(plain, flagged):
        with open(os.path.join(a["dir"], "3dbbox.json"), "rb") as f:
            want_json = f.read()
        with open(os.path.join(b["dir"], "3dbbox.json"), "rb") as f:
            assert f.read() == want_json, f"{a['name']}: 3dbbox.json changed with export_points"
        assert not os.path.exists(os.path.join(a["dir"], "points"))
        recs = json.loads(want_json)
        names = {f"{r['obj_id']}_{r['category_name'].replace(' ', '_')}.ply" for r in recs}
        assert len(names) == len(recs)
        pdir = os.path.join(b["dir"], "points")
        assert set(os.listdir(pdir) if os.path.isdir(pdir) else []) == names, a["name"]
        masks = kept_masks(a)
        depth = a["depth"]
        if depth_dtype == "u16":
            depth = np.where(depth == 0, np.float32(np.nan), depth.astype(np.float32) * np.float32(SCALE)).astype(np.float32)
        cloud = O.depth_to_points(depth[None], np.asarray(a["K"]))
        for r in recs:
            pts = cloud[masks[int(r["obj_id"])]]
            want = pts[np.isfinite(pts).all(axis=1)].astype(np.float32)
            got = read_ply(os.path.join(pdir, f"{r['obj_id']}_{r['category_name'].replace(' ', '_')}.ply"))
            np.testing.assert_array_equal(got, want, err_msg=f"{a['name']} obj {r['obj_id']}")
            assert len(want) >= 100
        assert len(recs) < len(a["annotations"])                      # the filter dropped something: no PLY for it (the set above)
        total += len(recs)
    return total


@pytest.mark.parametrize("mixed", [False, True], ids=["by size", "mixed frames"])
def test_the_full_cloud_under_subsample_and_ground(la, tmp_path, mixed):
    """the second phase (ground vectors, drawn indices) changes the fit, not the cloud: still the FULL mask's points"""
    from labelany3d_amd import fit_scenes as FS

    scenes = FS.synthetic_scenes(3, seed=21, H=240, W=320, mean_instances=14.0, rle_fraction=0.4, with_ground=True)[0]
    assert any("ground" in sc for sc in scenes)
    plain = run_tree(tmp_path / "plain", scenes, mixed_frames=mixed, subsample=True, rng=np.random.RandomState(5))
    flagged = run_tree(tmp_path / "flagged", scenes, mixed_frames=mixed, subsample=True, rng=np.random.RandomState(5), export_points=True)
    assert check_trees(plain, flagged) >= 6
    assert max(int(m.sum()) for sc in scenes for m in kept_masks(sc)) > 500      # a drawn instance is among them


def test_a_custom_points_dir_and_no_files_without_write(la, tmp_path):
    from labelany3d_amd import fit_scenes as FS

    scenes = scenes_of(None)[:3]
    placed = run_tree(tmp_path / "named", scenes, export_points=True, points_dir="clouds")
    assert any(os.path.isdir(os.path.join(sc["dir"], "clouds")) for sc in placed)
    assert not any(os.path.exists(os.path.join(sc["dir"], "points")) for sc in placed)
    dry = []
    for sc in scenes:
        d = os.path.join(str(tmp_path / "dry"), sc["name"])
        os.makedirs(d)
        dry.append(dict(sc, dir=d))
    got = list(FS.ScenePipeline(write=False, export_points=True).run(dry))
    assert len(got) == 3 and all(os.listdir(sc["dir"]) == [] for sc in dry)


def test_a_scene_that_was_yielded_has_its_clouds(la, tmp_path):
    """a consumer that stops after the first scene: that scene's json AND its PLYs were handed to the writers before it was yielded"""
    from labelany3d_amd import fit_scenes as FS

    scenes = scenes_of(None)
    placed = []
    for sc in scenes:
        d = os.path.join(str(tmp_path), sc["name"])
        os.makedirs(d)
        placed.append(dict(sc, dir=d))
    pipe = FS.ScenePipeline(mixed_frames=True, export_points=True)
    run = pipe.run(placed)
    first, recs = next(run)
    run.close()
    pipe.pool.shutdown(wait=True)
    assert len(recs) > 0
    names = {f"{r['obj_id']}_{r['category_name'].replace(' ', '_')}.ply" for r in recs}
    assert os.path.exists(os.path.join(first["dir"], "3dbbox.json"))
    assert set(os.listdir(os.path.join(first["dir"], "points"))) == names
