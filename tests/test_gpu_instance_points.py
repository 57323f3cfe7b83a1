"""GPU tests of the instance point clouds (``instance_points`` / ``instance_points_frames``; include/la3d.h "instance point clouds").

Comparison rules, the project's own: points within 1e-13 (rtol = atol) of ``oracle.la3d_oracle.depth_to_points`` - the figure of
tests/test_gpu_parity.py for ``unproject`` -, fitted records by ``assert_records`` (1e-9); everything else is exact equality (NaN
equal to NaN): against ``unproject`` of the same planes (the batched form: K is inverted in the kernel, as it is here), between the
u8 and the bit-plane call, between 16-bit planes and their unpacked float32 planes, between the frames call and the uniform call."""
import numpy as np
import pytest

from oracle import la3d_oracle as O

from . import frames_fault_rows as FR
from . import instance_points_cases as IC
from . import open_bits_frames_cases as FC
from .test_gpu_parity import assert_records, np_
from .test_hull_contract import hull_scene

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-13, atol=1e-13)
SENT = -12345.0


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def frame_case(H, W):
    """masks, shared planes through image_index, three cameras"""
    masks = IC.standard_masks(H, W)
    if (H, W) == (480, 640):
        masks = masks[[0, 3, 6, 7, 8, 9]]
    B = len(masks)
    return masks, IC.special_depth(3, H, W), IC.cameras(3, H, W), (np.arange(B) % 3).astype(np.int32)


def unprojected(la, depth, K):
    """the rows the clouds are cut from: la.unproject of the planes, (P, H*W, 3)"""
    return np_(la.unproject(np.ascontiguousarray(depth), K)).reshape(len(depth), -1, 3)


def check_cloud(ip, U, masks, ii, tag, oracle=None, pixels=True):
    """counts, offsets, rows and pixels of every instance, exactly; within 1e-13 of the oracle's rows where they are given"""
    B = len(masks)
    counts, offsets, pts, status = np_(ip.counts), np_(ip.offsets), np_(ip.points), np_(ip.status)
    want = masks.reshape(B, -1).sum(1)
    np.testing.assert_array_equal(counts, want, err_msg=tag)
    np.testing.assert_array_equal(offsets, np.concatenate([[0], np.cumsum(want)]), err_msg=tag)
    np.testing.assert_array_equal(status, 0, err_msg=tag)
    assert pts.shape == (offsets[-1], 3)
    for n in range(B):
        idx = np.flatnonzero(masks[n])
        np.testing.assert_array_equal(pts[offsets[n]:offsets[n + 1]], U[ii[n]][idx], err_msg=f"{tag}[{n}]")
        if pixels:
            np.testing.assert_array_equal(np_(ip.pixels)[offsets[n]:offsets[n + 1]], idx, err_msg=f"{tag}[{n}] pixels")
    if oracle is not None:
        np.testing.assert_allclose(pts, oracle, err_msg=tag, **TOL)


# ------------------------------------------------------------------------------------------
# 1. the uniform form: u8 planes and bit planes of the same masks
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", IC.FRAMES)
def test_u8_and_bit_planes_give_pts_mask(la, H, W):
    import torch

    masks, depth, K, ii = frame_case(H, W)
    U = unprojected(la, depth, K)
    for p in range(len(depth)):   # the single-frame entry (K inverted on the host by the same elimination) gives the same rows
        np.testing.assert_array_equal(np_(la.unproject(depth[p], K[p])).reshape(-1, 3), U[p])
    ref = IC.cloud_rule(depth, masks, K, ii)[0]
    ip = la.instance_points(depth, masks, K, image_index=ii, pixels=True)
    assert ip.points.dtype == torch.float64 and ip.offsets.dtype == torch.int64 and ip.counts.dtype == torch.int32
    check_cloud(ip, U, masks, ii, "u8", oracle=ref)
    empty = 0
    assert np_(ip.offsets)[empty] == np_(ip.offsets)[empty + 1]
    # an empty instance between non-empty ones
    order = np.array([1, 0, 3] if len(masks) == 10 else [1, 0, 2])
    mid = la.instance_points(depth, masks[order], K, image_index=ii[order])
    o = np_(mid.offsets)
    assert o[1] == o[2] and o[1] > 0 and o[3] > o[2]
    # the same masks as bit planes: rows padded to a multiple of 32 (depth padded by the call), and at the pitch of the frame
    for pad in (True, False):
        mb = la.pack_mask_bits(masks, frame_pad=pad)
        ib = la.instance_points(depth, mb, K, image_index=ii, pixels=True)
        for a, b in zip(ip, ib):
            assert torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0)), pad
    # float32 output: the cast of the float64 value
    i32 = la.instance_points(depth, masks, K, image_index=ii, out_dtype=torch.float32)
    assert i32.points.dtype == torch.float32 and i32.pixels is None
    np.testing.assert_array_equal(np_(i32.points), np_(ip.points).astype(np.float32))
    np.testing.assert_array_equal(np_(i32.offsets), np_(ip.offsets))


@pytest.mark.parametrize("B", [1, 7, 300])
def test_batch_sizes_private_planes_and_unaligned_u8(la, B):
    """B = 1, 7, 300 on 33 x 47 (odd width: the general u8 form and bit planes whose rows straddle words) with one private plane
    and camera per instance"""
    H, W = 33, 47
    base = IC.standard_masks(H, W)
    masks = base[(np.arange(B) * 7 + 3) % 10]
    depth, K = IC.special_depth(B, H, W, seed=B), IC.cameras(B, H, W)
    U = unprojected(la, depth, K)
    ip = la.instance_points(depth, masks, K, pixels=True)
    check_cloud(ip, U, masks, np.arange(B), f"B={B}", oracle=IC.cloud_rule(depth, masks, K)[0])
    ib = la.instance_points(depth, la.pack_mask_bits(masks, frame_pad=False), K, pixels=True)
    np.testing.assert_array_equal(np_(ib.points), np_(ip.points))
    np.testing.assert_array_equal(np_(ib.pixels), np_(ip.pixels))


def test_u8_planes_in_place_with_a_plane_stride_and_padded_columns(la):
    """the C entry on u8 planes that lie further apart than H*W at an odd base, with frame_width < W: set bytes in the padding columns
    are no pixels"""
    import ctypes as C

    import torch

    from labelany3d_amd import _lib

    H, W, fw, B = 33, 47, 41, 4
    masks = IC.standard_masks(H, W)[[3, 6, 7, 9]]
    depth, K = IC.special_depth(1, H, W), IC.cameras(1, H, W)
    stride = H * W + 13
    buf = torch.zeros(3 + B * stride, dtype=torch.uint8, device="cuda")
    for n in range(B):
        buf[3 + n * stride:3 + n * stride + H * W] = torch.as_tensor(masks[n].reshape(-1).astype(np.uint8) * (n + 1), device="cuda")
    d, k = torch.as_tensor(depth, device="cuda"), torch.as_tensor(K, device="cuda")
    ws = torch.empty(_lib.lib.la3d_instance_points_workspace_bytes(B, H, W) // 4, dtype=torch.int32, device="cuda")
    counts, offsets = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B + 1, dtype=torch.int64, device="cuda")
    a = _lib.CloudArgs(struct_size=C.sizeof(_lib.CloudArgs), B=B, H=H, W=W, frame_width=fw, depth=d.data_ptr(), mask=buf.data_ptr() + 3,
                       mask_plane_stride=stride, K=k.data_ptr(), counts=counts.data_ptr(), offsets=offsets.data_ptr(),
                       workspace=ws.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    assert _lib.lib.la3d_instance_point_offsets(C.byref(a)) == 0, _lib.lib.la3d_last_error()
    want = IC.cloud_rule(depth, masks, K, np.zeros(B, int), frame_width=fw)
    np.testing.assert_array_equal(np_(offsets), want[2])
    cap = int(want[2][-1])
    pts, pix = torch.empty((cap, 3), dtype=torch.float64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda")
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    a.points, a.pixels, a.status, a.capacity, a.out_is_f64 = pts.data_ptr(), pix.data_ptr(), status.data_ptr(), cap, 1
    assert _lib.lib.la3d_gather_instance_points(C.byref(a)) == 0, _lib.lib.la3d_last_error()
    np.testing.assert_allclose(np_(pts), want[0], **TOL)
    np.testing.assert_array_equal(np_(pix), want[1])
    np.testing.assert_array_equal(np_(status), 0)
    # B == 0: success, offsets[0] = 0
    offsets.fill_(77)
    z = _lib.CloudArgs(struct_size=C.sizeof(_lib.CloudArgs), B=0, H=H, W=W, offsets=offsets.data_ptr(), stream=a.stream)
    assert _lib.lib.la3d_instance_point_offsets(C.byref(z)) == 0 and _lib.lib.la3d_gather_instance_points(C.byref(z)) == 0
    assert np_(offsets)[0] == 0 and np_(offsets)[1] == 77


# ------------------------------------------------------------------------------------------
# 2. 16-bit depth
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "u16"])
def test_depth16_equals_the_float32_call_on_the_unpacked_planes(la, dtype):
    import torch

    for H, W in ((33, 47), (96, 224)):
        masks, depth, K, ii = frame_case(H, W)
        depth = depth.copy()
        depth[:, 2, 3] = 0.0                                          # uint16: a stored 0 is a hole
        d16 = la.pack_depth16(depth, dtype=dtype, scale=0.0025)
        assert d16.zero_is_hole
        up = la.unpack_depth16(d16)
        if dtype == "u16":
            assert torch.isnan(up[:, 2, 3]).all()
        for m in (masks, la.pack_mask_bits(masks)):
            got = la.instance_points(d16, m, K, image_index=ii, pixels=True)
            want = la.instance_points(up, m, K, image_index=ii, pixels=True)
            for a, b in zip(got, want):
                assert torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0)), (dtype, H, W)
            assert int(got.offsets[-1]) == masks.sum()
        if dtype == "u16":                                            # without the flag 0 is the depth 0.0
            got = la.instance_points(d16._replace(zero_is_hole=False), masks, K, image_index=ii)
            want = la.instance_points(la.unpack_depth16(d16._replace(zero_is_hole=False)), masks, K, image_index=ii)
            np.testing.assert_array_equal(np_(got.points), np_(want.points))


# ------------------------------------------------------------------------------------------
# 3. reference-subsample mode
# ------------------------------------------------------------------------------------------
def test_sample_idx_rows(la):
    import torch

    H, W = 200, 224
    depth, K = IC.special_depth(2, H, W), IC.cameras(2, H, W)
    masks = np.zeros((5, H, W), bool)
    for n, N in enumerate((137, 500, 501, 20011)):
        masks[n].reshape(-1)[11 * n + 5:11 * n + 5 + 2 * N:2] = True              # every other pixel: N of them
    masks[4, 20:150, 30:200] = np.random.RandomState(4).rand(130, 170) < 0.9       # ~ 20 000, many bands
    counts = masks.reshape(5, -1).sum(1)
    assert counts[:4].tolist() == [137, 500, 501, 20011] and counts[4] > 19000
    ii = np.array([0, 1, 0, 1, 0], np.int32)
    np.random.seed(5)
    idx = la.draw_sample_idx(counts)
    idx[2, 10] = idx[2, 11] = idx[2, 12] = 77                                     # a hand-made row: repeated ranks ...
    idx[3, 0], idx[3, 1], idx[3, 499] = 20011, -1, 20010                           # ... ranks outside the cloud, and the last rank
    want = IC.cloud_rule(depth, masks, K, ii, idx)
    U = unprojected(la, depth, K)
    for m in (masks, la.pack_mask_bits(masks)):
        ip = la.instance_points(depth, m, K, image_index=ii, sample_idx=idx, pixels=True)
        np.testing.assert_array_equal(np_(ip.counts), counts)
        np.testing.assert_array_equal(np_(ip.offsets), want[2])
        assert want[2].tolist() == [0, 137, 637, 1137, 1637, 2137]
        np.testing.assert_array_equal(np_(ip.status), 0)
        pts, pix, off = np_(ip.points), np_(ip.pixels), want[2]
        np.testing.assert_allclose(pts, want[0], **TOL)
        np.testing.assert_array_equal(pix, want[1])
        for n in range(5):
            cloud = U[ii[n]][np.flatnonzero(masks[n])]
            if counts[n] <= 500:
                np.testing.assert_array_equal(pts[off[n]:off[n + 1]], cloud)
            else:
                ok = (idx[n] >= 0) & (idx[n] < counts[n])
                np.testing.assert_array_equal(pts[off[n]:off[n + 1]][ok], cloud[idx[n][ok]])
                assert np.isnan(pts[off[n]:off[n + 1]][~ok]).all() and (pix[off[n]:off[n + 1]][~ok] == -1).all()
        np.testing.assert_array_equal(pts[off[2] + 10], pts[off[2] + 11])
        np.testing.assert_array_equal(pts[off[2] + 10], pts[off[2] + 12])
        assert np.isnan(pts[off[3]:off[3] + 2]).all() and not np.isnan(pts[off[3] + 499]).all()
    assert isinstance(ip.points, torch.Tensor)


# ------------------------------------------------------------------------------------------
# 4. capacity and masks that change between the stages
# ------------------------------------------------------------------------------------------
def _sentinel_out(la, cap, B):
    import torch

    return (torch.full((cap, 3), SENT, dtype=torch.float64, device="cuda"), torch.full((cap,), int(SENT), dtype=torch.int32, device="cuda"),
            torch.full((B,), -9, dtype=torch.int32, device="cuda"))


def test_capacity_one_row_short(la):
    H, W = 96, 224
    masks, depth, K, ii = frame_case(H, W)
    B = len(masks)                                                      # (the last instance, the blob, is not empty)
    full = la.instance_points(depth, masks, K, image_index=ii, pixels=True)
    total = int(full.offsets[-1])
    off = np_(full.offsets)
    room = 64
    out = _sentinel_out(la, total + room, B)
    ip = la.instance_points(depth, masks, K, image_index=ii, capacity=total - 1, pixels=True, _out=out)
    status = np_(ip.status)
    last = B - 1
    assert status[last] == 1 and (status[:last] == 0).all()
    pts, pix = np_(out[0]), np_(out[1])
    np.testing.assert_array_equal(pts[:off[last]], np_(full.points)[:off[last]])
    np.testing.assert_array_equal(pix[:off[last]], np_(full.pixels)[:off[last]])
    assert (pts[off[last]:] == SENT).all() and (pix[off[last]:] == int(SENT)).all()
    # an exact capacity fits, and never synchronises on its way
    out = _sentinel_out(la, total + room, B)
    ip = la.instance_points(depth, masks, K, image_index=ii, capacity=total, pixels=True, _out=out)
    np.testing.assert_array_equal(np_(ip.status), 0)
    np.testing.assert_array_equal(np_(out[0])[:total], np_(full.points))
    assert (np_(out[0])[total:] == SENT).all()


def test_masks_changed_between_the_stages(la):
    """offsets (and the workspace) come from other masks: the affected instances report status 2 and nothing is written outside
    any instance's own range"""
    import torch

    H, W = 96, 224
    masks, depth, K, ii = frame_case(H, W)
    B = len(masks)
    other = masks.copy()
    other[4] = masks[5]                                                # the row became a column: fewer pixels
    other[7] = masks[7] | masks[6]                                     # many more pixels
    other[9] = np.roll(masks[9], 3 * W + 5)                            # as many pixels, elsewhere (other bands)
    changed = [4, 7, 9]
    plan_ip, ws = la.instance_points(depth, masks, K, image_index=ii, pixels=True, _with_plan=True)
    off = np_(plan_ip.offsets)
    total = int(off[-1])
    out = _sentinel_out(la, total + 64, B)
    m2 = torch.as_tensor(other.view(np.uint8), device="cuda")
    ip = la.instance_points(depth, m2, K, image_index=ii, pixels=True, _plan=(plan_ip.counts, plan_ip.offsets, ws), _out=out)
    status = np_(ip.status)
    assert (status[changed] == 2).all() and (np.delete(status, changed) == 0).all(), status
    pts, pix = np_(out[0]), np_(out[1])
    assert (pts[total:] == SENT).all() and (pix[total:] == int(SENT)).all()
    U = unprojected(la, depth, K)
    for n in range(B):
        rows, prow = pts[off[n]:off[n + 1]], pix[off[n]:off[n + 1]]
        if n not in changed:
            np.testing.assert_array_equal(rows, np_(plan_ip.points)[off[n]:off[n + 1]])
            continue
        # whatever was written inside the range is a point of a pixel of the NEW mask; the rest kept the sentinel
        written = prow != int(SENT)
        assert other[n].reshape(-1)[prow[written]].all()
        np.testing.assert_array_equal(rows[written], U[ii[n]][prow[written]])
        assert (rows[~written] == SENT).all()


# ------------------------------------------------------------------------------------------
# 5. the frames form
# ------------------------------------------------------------------------------------------
FSIZES = ((96, 224), (33, 47), (100, 214), (5, 13), (480, 640), (40, 70))
NO_INSTANCES = 5


def frames_case(seed=0):
    rs = np.random.RandomState(seed)
    labels, stacks, ids = [], [], []
    for p, (H, W) in enumerate(FSIZES):
        lab = rs.randint(0, 4, (max(H // 6, 1), max(W // 9, 1))).repeat(6, 0).repeat(9, 1)
        lab = np.pad(lab, ((0, max(0, H - lab.shape[0])), (0, max(0, W - lab.shape[1]))), mode="edge")[:H, :W].astype(np.uint8)
        lab[rs.rand(H, W) < 0.05] = 3
        lab[H - 1, W - 3:] = 2
        labels.append(lab)
        want = [] if p == NO_INSTANCES else [1, 2, 3]
        ids.append(want)
        stacks.append(np.stack([lab == i for i in want]) if want else np.zeros((0, H, W), bool))
    img = np.repeat(np.arange(len(FSIZES)), [len(x) for x in ids]).astype(np.int32)
    depth = [IC.special_depth(1, H, W, seed=10 + p)[0] for p, (H, W) in enumerate(FSIZES)]
    K = np.stack([IC.cameras(1, H, W)[0] for H, W in FSIZES])
    return labels, stacks, ids, img, depth, K


def to_u16(depth, scale):
    with np.errstate(invalid="ignore"):
        return [np.where(np.isfinite(d) & (d > 0), np.minimum(np.rint(d / np.float32(scale)), 65535), 0).astype(np.uint16) for d in depth]


@pytest.mark.parametrize("source", ["labels", "masks"])
@pytest.mark.parametrize("depth_kind", ["f32", "u16"])
def test_frames_form(la, source, depth_kind):
    import torch

    labels, stacks, ids, img, depth, K = frames_case()
    B = len(img)
    if depth_kind == "u16":
        words = to_u16(depth, 0.001)
        pf = la.pack_frames(words, dtype="u16", scale=0.001)
        depth = [np_(la.unpack_depth16(la.Depth16(torch.as_tensor(w, device="cuda"), 0.001, True))) for w in words]
    else:
        pf = la.pack_frames(depth)
    fb = la.pack_label_bits_frames(la.pack_label_frames(labels), ids) if source == "labels" else la.pack_mask_bits_frames(la.pack_mask_frames(stacks))
    perm = np.random.RandomState(3).permutation(B)
    t = torch.as_tensor(perm, device="cuda")
    fb = fb._replace(offsets=fb.offsets[t].contiguous(), image_index=fb.image_index[t].contiguous(), area=fb.area[t].contiguous())
    ip = la.instance_points_frames(pf, fb, K, pixels=True)
    np.testing.assert_array_equal(np_(ip.status), 0)
    off, pts, pix = np_(ip.offsets), np_(ip.points), np_(ip.pixels)
    per = [list(stacks[p]) for p in range(len(FSIZES))]
    masks_of = [m for p in range(len(FSIZES)) for m in per[p]]                # in image order
    np.testing.assert_array_equal(np_(ip.counts), [masks_of[b].sum() for b in perm])
    np.testing.assert_array_equal(np_(ip.counts), np_(fb.area))
    uniform = {}
    for p, (H, W) in enumerate(FSIZES):
        if len(stacks[p]):
            uniform[p] = la.instance_points(depth[p], stacks[p], K[p], pixels=True)
    first = np.concatenate([[0], np.cumsum([len(x) for x in ids])])
    for row, b in enumerate(perm):
        p = int(img[b])
        k = int(b - first[p])
        u = uniform[p]
        uo = np_(u.offsets)
        got = pts[off[row]:off[row + 1]]
        np.testing.assert_array_equal(got, np_(u.points)[uo[k]:uo[k + 1]], err_msg=f"row {row} image {p}")      # exact against the uniform call
        np.testing.assert_array_equal(pix[off[row]:off[row + 1]], np_(u.pixels)[uo[k]:uo[k + 1]])
        np.testing.assert_allclose(got, O.depth_to_points(depth[p][None], K[p])[stacks[p][k]], **TOL)            # the oracle on the unpadded frame
    # float32 output and one shared camera
    i32 = la.instance_points_frames(pf, fb, K[0], out_dtype=torch.float32)
    one = la.instance_points_frames(pf, fb, K[0])
    np.testing.assert_array_equal(np_(i32.points), np_(one.points).astype(np.float32))


def test_frames_form_refuses_broken_rows_on_the_device(la):
    import torch

    labels, stacks, ids, img, depth, K = frames_case(1)
    B = len(img)
    pf = la.pack_frames(depth)
    fb = la.pack_mask_bits_frames(la.pack_mask_frames(stacks))
    good = la.instance_points_frames(pf, fb, K, pixels=True)
    goff = np_(good.offsets)
    BROKEN = 2                                                       # image 2 gets a pitch that is no multiple of 32
    table = pf.table.clone()
    table[BROKEN, 3] = 214
    ii = np_(fb.image_index).copy()
    offs = np_(fb.offsets).copy()
    outside, misaligned = int(np.flatnonzero(img == 0)[1]), int(np.flatnonzero(img == 4)[0])
    ii[outside] = 99
    offs[misaligned] += 2
    refused = (img == BROKEN)
    refused[[outside, misaligned]] = True
    bad_pf = pf._replace(table=table)
    bad_fb = fb._replace(offsets=torch.as_tensor(offs, device="cuda"), image_index=torch.as_tensor(ii, device="cuda"))
    total = int(goff[-1])
    out = _sentinel_out(la, total, B)
    ip = la.instance_points_frames(bad_pf, bad_fb, K, pixels=True, capacity=total, _out=out)
    status, counts, off = np_(ip.status), np_(ip.counts), np_(ip.offsets)
    np.testing.assert_array_equal(status[refused], 5)
    np.testing.assert_array_equal(status[~refused], 0)
    assert (counts[refused] == 0).all() and (np.diff(off)[refused] == 0).all()
    np.testing.assert_array_equal(counts[~refused], np_(good.counts)[~refused])
    pts, pix = np_(out[0]), np_(out[1])
    for b in np.flatnonzero(~refused):
        np.testing.assert_array_equal(pts[off[b]:off[b + 1]], np_(good.points)[goff[b]:goff[b + 1]])
        np.testing.assert_array_equal(pix[off[b]:off[b + 1]], np_(good.pixels)[goff[b]:goff[b + 1]])
    assert (pts[off[-1]:] == SENT).all() and (pix[off[-1]:] == int(SENT)).all() and off[-1] < total
    # the shared case table (tests/frames_fault_rows.py), one fault per row: the table, the planes and the depth have pad in front
    # and behind, so a defect shows as a row too many or a wrong status, never as a fault.  (The entry takes no length of the planes.)
    sizes = [h * FR.padded(w) for h, w in FR.GOOD]
    fc = FR.case(end_check=False, depth_offsets=(0, sizes[0], sizes[0] + sizes[1]))
    rs = np.random.RandomState(6)
    ms = {n: rs.rand(*FR.GOOD[fc.rows[n][0]]) < 0.3 for n in fc.good}
    d = FR.on_device(fc, FR.input_words(fc, rs, lambda n, h, w: FC.frame_words(ms[n])))
    dbuf = torch.as_tensor(rs.uniform(0.5, 10.0, FR.PAD + sum(sizes) + FR.PAD).astype(np.float32), device="cuda")
    fpf = la.PackedFrames(dbuf[FR.PAD:FR.PAD + sum(sizes)], d.table, fc.table[1:1 + fc.P], fc.H, fc.W, list(FR.GOOD) + [(8, 32)] * (fc.P - 3))
    fK = np.stack([IC.cameras(1, h, w)[0] for h, w in fpf.sizes])
    good = la.instance_points_frames(fpf, FR.frame_bits(la, fc, d, fc.good), fK, pixels=True)      # the call without the bad rows
    goff = np_(good.offsets)
    np.testing.assert_array_equal(np_(good.counts), [ms[n].sum() for n in fc.good])
    total = int(goff[-1])
    out = _sentinel_out(la, total + 16, fc.B)
    ip = la.instance_points_frames(fpf, FR.frame_bits(la, fc, d), fK, pixels=True, capacity=total + 16, _out=out)
    status, counts, off = np_(ip.status), np_(ip.counts), np_(ip.offsets)
    for n, (img, fault) in enumerate(fc.rows):
        assert (status[n], counts[n] == 0, off[n + 1] - off[n] == 0) == ((5, True, True) if fault else (0, False, False)), (n, fault)
    pts, pix = np_(out[0]), np_(out[1])
    for k, n in enumerate(fc.good):
        np.testing.assert_array_equal(pts[off[n]:off[n + 1]], np_(good.points)[goff[k]:goff[k + 1]], err_msg=f"row {n}")
        np.testing.assert_array_equal(pix[off[n]:off[n + 1]], np_(good.pixels)[goff[k]:goff[k + 1]], err_msg=f"row {n}")
    assert off[-1] == total and (pts[total:] == SENT).all() and (pix[total:] == int(SENT)).all()


# ------------------------------------------------------------------------------------------
# 6. composition: the clouds are what fit_points takes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grounded", [False, True])
def test_fit_points_on_the_clouds_gives_the_fitted_records(la, grounded):
    B, H, W = 12, 96, 224
    depth, masks, K = hull_scene(31, B, H, W)
    ground = None
    if grounded:
        rs = np.random.RandomState(2)
        ground = np.column_stack([0.1 * rs.randn(B), -1.0 + 0.1 * rs.randn(B), 0.1 * rs.randn(B), rs.uniform(1, 2, B)])
    ip = la.instance_points(depth, masks, K)
    got = la.fit_points((ip.points, ip.offsets), ground)
    want = la.fit_instances(depth, masks, K, ground)
    np.testing.assert_array_equal(np_(got[1]), np_(want[1]))
    assert (np_(want[1]) == 0).all()
    assert_records(np_(got[0]), np_(want[0]), "full mask", gap=np_(want[2])[:, 3])
    # and with one sample_idx given to both
    np.random.seed(9)
    idx = la.draw_sample_idx(ip.counts)
    assert (np_(ip.counts) > 500).any()
    sp = la.instance_points(depth, masks, K, sample_idx=idx)
    assert int(sp.offsets[-1]) == np.minimum(np_(ip.counts), 500).sum()
    got = la.fit_points((sp.points, sp.offsets), ground)                # (the rows are drawn already: no sample_idx here)
    want = la.fit_instances(depth, masks, K, ground, sample_idx=idx)
    np.testing.assert_array_equal(np_(got[1]), np_(want[1]))
    assert_records(np_(got[0]), np_(want[0]), "sampled", gap=np_(want[2])[:, 3])


# ------------------------------------------------------------------------------------------
# 7. the two stages captured into a graph
# ------------------------------------------------------------------------------------------
def test_two_stage_chain_captured_into_a_graph(la):
    """count -> scan -> status -> gather: one linear chain on one stream, captured once with a fixed capacity and replayed twice with
    other masks written into the same buffers"""
    import torch

    H, W = 96, 224
    dev = torch.device("cuda", 0)
    masks0, depth, K, ii = frame_case(H, W)
    B = len(masks0)
    cap = 3 * H * W
    m = torch.as_tensor(masks0.view(np.uint8), device=dev)
    d, k, i = torch.as_tensor(depth, device=dev), torch.as_tensor(K, device=dev), torch.as_tensor(ii, device=dev)
    out = _sentinel_out(la, cap, B)
    side = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        la.instance_points(d, m, k, image_index=i, capacity=cap, pixels=True, _out=out, stream=side)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            held = la.instance_points(d, m, k, image_index=i, capacity=cap, pixels=True, _out=out, stream=torch.cuda.current_stream())
    U = unprojected(la, depth, K)
    for seed in (1, 2):
        masks = IC.standard_masks(H, W, seed=seed)[np.random.RandomState(seed).permutation(B)]
        m.copy_(torch.as_tensor(masks.view(np.uint8), device=dev))
        for t in out:
            t.fill_(int(SENT))
        g.replay()
        torch.cuda.synchronize()
        off = np_(held.offsets)
        np.testing.assert_array_equal(np_(held.status), 0)
        np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(masks.reshape(B, -1).sum(1))]))
        for n in range(B):
            idx = np.flatnonzero(masks[n])
            np.testing.assert_array_equal(np_(out[0])[off[n]:off[n + 1]], U[ii[n]][idx])
            np.testing.assert_array_equal(np_(out[1])[off[n]:off[n + 1]], idx)
        assert (np_(out[0])[off[-1]:] == SENT).all()
