"""GPU tests of the instances that get NO box from the instance engine, path by path, and of the two branches of its tile list that
no other test runs.

A refused or dropped instance has four outputs, and each case pins all of them exactly: the status, the aux tuple, an all-NaN
39-double record and - the call is made with ``image_size`` - all-NaN ``boxes2d``.  The expected aux tuples are the constants of
the two writers (la3d_device.hpp: write_no_box / write_no_box_axis), not recordings:

  refused before anything was counted (frame row, no per-column structure, frame outside the tiled path)   (NaN, 0, NaN, NaN)
  dropped by the fused filter                                                                             (NaN, 0, area, NaN)
  refused by the hull finish (more candidates than it holds)                                              (NaN, n_valid, n_masked, NaN)

(The axis stage's rejections - status 1, 2, 3: aux = (yaw, n_valid, n_masked, gap) - are pinned by
tests/test_gpu_parity.py::test_status_codes_batched and the campaigns.)  Frames are small: every case is one launch of a few
workgroups.  The tile-list cases are checked against the oracle with ``assert_records`` at the tolerances it carries."""
import numpy as np
import pytest

from oracle import la3d_oracle as O
from oracle import poly_oracle as P

from .conftest import SCHED
from .test_gpu_parity import assert_records

pytestmark = pytest.mark.gpu

NAN = np.nan


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def np_(t):
    return t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()


def camera(H, W):
    return np.array([[0.8 * W, 0, W / 2.0], [0, 0.8 * W, H / 2.0], [0, 0, 1]])


def assert_no_box(res, n, status, aux, tag):
    """res: dict with boxes / status / aux / boxes2d; instance n has no box: the four outputs, exactly"""
    assert int(np_(res["status"])[n]) == status, f"{tag}: status"
    np.testing.assert_array_equal(np_(res["aux"])[n], np.asarray(aux, float), err_msg=f"{tag}: aux")   # (NaN == NaN here: the pattern and the finite entries)
    rec, b2 = np_(res["boxes"])[n], np_(res["boxes2d"])[n]
    assert rec.shape == (39,) and np.isnan(rec).all(), f"{tag}: record"
    assert b2.shape == (8,) and np.isnan(b2).all(), f"{tag}: boxes2d"


def as_dict(t):
    """the tuple of fit_instances_bits(filter=..., image_size=...)"""
    return dict(zip(("boxes", "status", "aux", "stats", "boxes2d"), t))


# ------------------------------------------------------------------------------------------
# the fused filter drops the instance: status 6, aux[2] = the mask's area
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["rle", "poly", "bits"])
def test_filter_drop(la, source):
    H, W, B = 16, 64, 2
    depth = np.random.RandomState(1).uniform(1, 5, (B, H, W)).astype(np.float32)
    segs = [[[10, 5, 11, 5, 11, 6, 10, 6]], [[40, 9, 41, 9, 41, 10, 40, 10]]]   # two 2 x 2 squares (cv2.fillPoly fills the outline's pixels)
    masks = np.stack([P.create_boolean_mask_from_polygon((W, H), s)[0] for s in segs])
    assert masks.reshape(B, -1).sum(1).tolist() == [4, 4] and masks[0, 5:7, 10:12].all() and masks[1, 9:11, 40:42].all()
    K = camera(H, W)
    if source == "rle":
        res = la.fit_instances_ex(depth, K, rles=[O.rle_encode(m) for m in masks], filter=True, image_size=(W, H))
    elif source == "poly":
        res = la.fit_instances_ex(depth, K, polys=la.pack_polygons(segs, H, W), filter=True, image_size=(W, H))
    else:
        res = as_dict(la.fit_instances_bits(depth, la.pack_mask_bits(masks), K, filter=True, image_size=(W, H)))
    for n in range(B):
        assert_no_box(res, n, 6, (NAN, 0.0, 4.0, NAN), f"{source}[{n}]")
    assert (np_(res["stats"])[:, 0] == 4).all()


# ------------------------------------------------------------------------------------------
# a frames call refuses a frame row: status 5 before anything is read through the row
# ------------------------------------------------------------------------------------------
def test_frames_call_refuses_a_frame_row(la):
    import torch

    sizes = [(16, 64), (24, 96)]
    rs = np.random.RandomState(2)
    depth = [rs.uniform(1, 5, s).astype(np.float32) for s in sizes]
    K = np.stack([camera(h, w) for h, w in sizes])
    masks = [np.zeros(s, bool) for s in sizes]
    masks[0][3:12, 8:40] = True
    masks[1][4:20, 10:70] = True
    pf = la.pack_frames(depth)
    table = pf.table_host.copy()
    table["H"][0] = 0                                       # zero rows: outside the contract of la3d_frame (and a row that addresses nothing)
    words = torch.as_tensor(np.ascontiguousarray(table).view(np.int32).reshape(len(sizes), 6).copy(), device="cuda")
    res = la.fit_instances_frames(pf._replace(table=words, table_host=table), K, rles=[O.rle_encode(m) for m in masks],
                                  image_index=np.array([0, 1], np.int32), proj=True)
    assert_no_box(res, 0, 5, (NAN, 0.0, NAN, NAN), "refused row")
    assert int(np_(res["status"])[1]) == 0 and np.isfinite(np_(res["boxes"])[1]).all()   # the conforming frame beside it is fitted
    assert np_(res["aux"])[1, 2] == masks[1].sum()


# ------------------------------------------------------------------------------------------
# full-mask hull: no per-column structure (ground plane), a frame outside the tiled path, too many candidates
# ------------------------------------------------------------------------------------------
def test_hull_full_mask_with_ground_plane(la):
    H, W, B = 16, 64, 2
    depth = np.random.RandomState(3).uniform(1, 5, (B, H, W)).astype(np.float32)
    masks = np.zeros((B, H, W), bool)
    masks[:, 3:12, 8:40] = True
    ground = np.array([[0.02, -0.98, 0.1, 1.5], [NAN] * 4])
    res = la.fit_instances_ex(depth, camera(H, W), masks=masks, ground=ground, image_size=(W, H), method="convex_hull")
    assert_no_box(res, 0, 5, (NAN, 0.0, NAN, NAN), "ground plane")
    # (on a frame this small the instance without ground is refused by the same test for another reason: the per-column ranges -
    # 2 x 64 words = 512 B - do not fit behind the tile entries in the 128 B of the bit image)
    assert_no_box(res, 1, 5, (NAN, 0.0, NAN, NAN), "no room for the column ranges")


def test_hull_full_mask_width_no_multiple_of_32(la):
    """u8 planes 40 columns wide, handed over as they are (fit_instances_ex does not pad u8 planes): the frame is outside the tiled
    path, one workgroup of 256 threads refuses the B = 3 instances - the bound inst >= B lies inside it."""
    H, W, B = 8, 40, 3
    depth = np.random.RandomState(4).uniform(1, 5, (B, H, W)).astype(np.float32)
    masks = np.zeros((B, H, W), bool)
    masks[:, 1:7, 4:30] = True
    res = la.fit_instances_ex(depth, camera(H, W), masks=masks, image_size=(W, H), method="convex_hull")
    assert np_(res["status"]).shape == (B,)
    for n in range(B):
        assert_no_box(res, n, 5, (NAN, 0.0, NAN, NAN), f"W=40[{n}]")


def test_hull_finish_with_more_candidates_than_it_holds(la):
    """72 x 1056, the mask = the first two rows, the two rows' depths differ in every column: two candidates per column, 2112 against
    the 2048 the hull finish holds (HULL_MAX).  The 33 active tiles leave room for the per-column ranges behind them
    (33 * 32 + 2 * 1056 * 4 = 9504 = the bit image's bytes), so the instance takes the separable walk and reaches the finish."""
    H, W = 72, 1056
    depth = np.full((1, H, W), 4.0, np.float32)
    depth[0, 0] = 2.0 + 0.001 * np.arange(W)
    depth[0, 1] = 3.5 + 0.001 * np.arange(W)
    assert (depth[0, 0] != depth[0, 1]).all() and 2 * W > 2048
    masks = np.zeros((1, H, W), bool)
    masks[0, :2] = True
    res = la.fit_instances_ex(depth, camera(H, W), masks=masks, image_size=(W, H), method="convex_hull")
    assert_no_box(res, 0, 5, (NAN, 2.0 * W, 2.0 * W, NAN), "2112 candidates")


# ------------------------------------------------------------------------------------------
# the tile list's two-pass form: more than 2048 tiles, so that a wave owns more than 256
# (a frame height with H % 8 != 0 - the clamped classification - is run by tests/test_gpu_parity.py::test_odd_frame_sizes[100-96-instance])
# ------------------------------------------------------------------------------------------
def test_tile_list_two_pass_form_vs_oracle(la, monkeypatch):
    monkeypatch.setattr(SCHED(), "engine", "instance")
    H, W, B = 520, 1024, 2
    assert (W // 32) * ((H + 7) // 8) > 2048
    rs = np.random.RandomState(H * W)
    depth = rs.uniform(1, 5, (B, H, W)).astype(np.float32)
    masks = np.zeros((B, H, W), bool)
    masks[0, 37:300, 100:613] = True
    masks[1] = rs.rand(H, W) < 0.004                          # scattered pixels: many active tiles, none full
    K = camera(H, W)
    ground = np.array([[0.1, -0.9, 0.2, 1.0], [NAN] * 4])   # (one instance with a ground plane - two passes -, one on the separable path)
    boxes, status, aux = la.fit_instances(depth, masks, K, ground=ground)
    ref, rst, _, rn = O.fit_instances(depth, masks, K, ground=[ground[0], None])
    assert (np_(status) == rst).all() and (rst == 0).all()
    assert_records(np_(boxes), ref, "520x1024", gap=np_(aux)[:, 3])
    np.testing.assert_array_equal(np_(aux)[:, 1], rn)
    np.testing.assert_array_equal(np_(aux)[:, 2], masks.reshape(B, -1).sum(1))
