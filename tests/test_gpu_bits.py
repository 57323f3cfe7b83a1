"""GPU tests of the bit-plane mask source (include/la3d.h "masks as bit planes"): the packers against ``np.packbits``, and
``fit_instances_bits`` / ``InstanceFitter.run_bits`` against the oracle, the run-length entry and the u8 entry pinned to the instance
engine.  Comparison rules are the suite's own: ``assert_records`` against the oracle, ``assert_hull_records`` for hull records, and
between two entries of one engine status / ``aux[:, 1:3]`` / filter statistics equal and records to ``rtol = atol = 1e-12`` (the
rule of ``test_fit_from_rle_equals_fit_from_planes``).  The bit planes a fit is fed with are packed HERE with ``np.packbits``, never
with the code under test."""
import numpy as np
import pytest

from oracle import la3d_oracle as O

from .conftest import SCHED
from .test_gpu_hull_instances import check_against_oracle as check_hull_against_oracle
from .test_gpu_hull_instances import hull_scene
from .test_gpu_parity import assert_records

pytestmark = pytest.mark.gpu

K640 = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
K224 = np.array([[180.0, 0, 112], [0, 180.0, 48], [0, 0, 1]])


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def np_(t):
    return t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()


def padded(W):
    return (W + 31) // 32 * 32


def packbits(masks, W_out=None):
    """(B,H,W) -> the expected words (B, ceil(H*W_out/32)) uint32: np.packbits, LSB first, of the rows padded with zeros to W_out"""
    masks = np.asarray(masks) != 0
    B, H, W = masks.shape
    W_out = W if W_out is None else W_out
    m = np.zeros((B, H, W_out), bool)
    m[:, :, :W] = masks
    by = np.packbits(m.reshape(B, -1), axis=1, bitorder="little")
    by = np.pad(by, ((0, 0), (0, (-by.shape[1]) % 4)))
    return np.ascontiguousarray(by).view("<u4")


def host_bits(masks, pad=True):
    """the MaskBits tuple of masks, packed on the host and uploaded"""
    import torch

    B, H, W = masks.shape
    W_out = padded(W) if pad else W
    t = torch.as_tensor(packbits(masks, W_out).view(np.int32), device="cuda")
    return (t, H, W_out, W)


def words(t):
    return np_(t).view(np.uint32)


def zoo(rs, H, W):
    """the mask zoo of tests/test_gpu_masks.py::test_rle_decode_random_masks"""
    masks = np.zeros((12, H, W), bool)
    masks[9, :, 3:W - 5] = True
    masks[9, :H // 3, 3] = False
    masks[9, H // 2:, W - 6] = False
    masks[10, :, 1:2 + W // 3] = True
    masks[10, H - 1, 1] = False
    masks[11, H - 1, :] = True
    masks[11, 0, ::2] = True
    for i in range(5):
        h, w = rs.randint(1, H + 1), rs.randint(1, W + 1)
        r0, c0 = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
        masks[i, r0:r0 + h, c0:c0 + w] = True
    masks[5] = rs.rand(H, W) < 0.5
    masks[6] = True
    masks[7] = False
    masks[8, :, W // 2] = True
    return masks


def rle_masks(B, H, W, seed=77):
    """the masks of tests/test_gpu_masks.py::test_fit_from_rle_equals_fit_from_planes: rectangles, an ellipse, 2 % random, one empty"""
    rs = np.random.RandomState(seed)
    depth = rs.uniform(0.5, 10, (B, H, W)).astype(np.float32)
    masks = np.zeros((B, H, W), bool)
    for i in range(B - 3):
        h, w = rs.randint(8, min(301, H + 1)), rs.randint(8, min(331, W + 1))
        r0, c0 = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
        masks[i, r0:r0 + h, c0:c0 + w] = True
    vv, uu = np.mgrid[0:H, 0:W]
    masks[B - 3] = ((uu - 0.47 * W) ** 2 / (0.15 * W) ** 2 + (vv - 0.42 * H) ** 2 / (0.13 * H) ** 2) < 1.0
    masks[B - 2] = rs.rand(H, W) < 0.02
    ground = np.array([[0.02, -0.98, 0.1, 1.5]] * B) + 0.03 * rs.randn(B, 4)
    return depth, masks, ground


def oracle(depth, masks, K, ground=None, sample_idx=None, depth_index=None):
    ref, st, _, nv = O.fit_instances(depth, masks, K, ground=ground, sample_idx=sample_idx, depth_index=depth_index)
    if ground is not None and np.isnan(np.asarray(ground)[:, 0]).any():   # a NaN row means "no ground" for that instance (la3d.h)
        r0, s0, _, n0 = O.fit_instances(depth, masks, K, ground=None, sample_idx=sample_idx, depth_index=depth_index)
        free = np.isnan(np.asarray(ground)[:, 0])
        ref[free], st[free], nv[free] = r0[free], s0[free], n0[free]
    return ref, st, nv


def check_oracle(got, depth, masks, K, tag, **kw):
    boxes, status, aux = (np_(t) for t in got[:3])
    ref, st, nv = oracle(depth, masks, K, **kw)
    np.testing.assert_array_equal(status, st, err_msg=f"{tag} status")
    ok = st == 0
    assert np.isnan(boxes[~ok]).all(), tag
    assert_records(boxes[ok], ref[ok], tag, gap=aux[ok, 3])
    np.testing.assert_array_equal(aux[ok, 1], nv[ok], err_msg=f"{tag} n_valid")
    np.testing.assert_array_equal(aux[:, 2], np.asarray(masks).reshape(len(masks), -1).sum(1), err_msg=f"{tag} n_masked")
    return status


def same_engine(got, other, tag):
    """two entries of the same engine: status, aux[:, 1:3] equal, records to rtol = atol = 1e-12"""
    b0, s0, a0 = (np_(t) for t in got[:3])
    b1, s1, a1 = (np_(t) for t in other[:3])
    np.testing.assert_array_equal(s0, s1, err_msg=f"{tag} status")
    np.testing.assert_array_equal(a0[:, 1:3], a1[:, 1:3], err_msg=f"{tag} aux")
    np.testing.assert_allclose(np.nan_to_num(b0, nan=-7.0), np.nan_to_num(b1, nan=-7.0), rtol=1e-12, atol=1e-12, err_msg=f"{tag} records")


def u8_on_instance_engine(la, *a, **k):
    SCHED().engine = "instance"
    try:
        return la.fit_instances(*a, **k)
    finally:
        SCHED().engine = None


def rle_on_instance_engine(la, depth, masks, K, **k):
    """the run-length entry of the same masks, pinned to the engine bit planes run on"""
    SCHED().engine = "instance"
    try:
        return la.fit_instances_rle(depth, [O.rle_encode(m) for m in masks], K, **k)
    finally:
        SCHED().engine = None


# ------------------------------------------------------------------------------------------
# 4. packers, unpacker, statistics
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(480, 640), (96, 224), (64, 96), (37, 53), (100, 214), (33, 427), (8, 32), (5, 7)])
def test_pack_mask_bits_equals_packbits(la, H, W):
    import torch

    rs = np.random.RandomState(H * 7 + W)
    masks = zoo(rs, H, W)
    B = len(masks)
    want_pad, want_raw = packbits(masks, padded(W)), packbits(masks)
    for name, src in (("bool", masks), ("0/1", masks.astype(np.uint8)), ("255", (masks * 255).astype(np.uint8)),
                      ("torch bool", torch.as_tensor(masks, device="cuda")), ("mixed", (masks * rs.randint(1, 256, masks.shape)).astype(np.uint8))):
        mb = la.pack_mask_bits(src)
        assert (mb.H, mb.W, mb.frame_width) == (H, padded(W), W) and mb.bits.dtype == torch.int32
        np.testing.assert_array_equal(words(mb.bits), want_pad, err_msg=f"{name} padded")
        mb = la.pack_mask_bits(src, frame_pad=False)
        assert (mb.H, mb.W, mb.frame_width) == (H, W, W)
        np.testing.assert_array_equal(words(mb.bits), want_raw, err_msg=f"{name} unpadded")
    # round trip
    for pad in (True, False):
        back = la.unpack_mask_bits(la.pack_mask_bits(masks, frame_pad=pad))
        assert back.dtype == torch.bool and tuple(back.shape) == (B, H, W)
        np.testing.assert_array_equal(np_(back), masks)
    back = la.unpack_mask_bits(host_bits(masks))
    np.testing.assert_array_equal(np_(back), masks)


def test_pack_mask_bits_strided_sliced_and_misaligned_planes(la):
    import torch

    rs = np.random.RandomState(5)
    H, W, B = 64, 96, 9
    masks = rs.rand(B, H, W) < 0.4
    want = packbits(masks)
    big = torch.zeros((2 * B + 1, H, W), dtype=torch.uint8, device="cuda")
    big[1::2][:B] = torch.as_tensor(masks.view(np.uint8), device="cuda") * 3
    src = big[1::2][:B]                                  # every second plane of a larger stack: plane stride 2 H W
    assert not src.is_contiguous()
    np.testing.assert_array_equal(words(la.pack_mask_bits(src).bits), want)
    np.testing.assert_array_equal(words(la.pack_mask_bits(big[3:3 + B]).bits), packbits(np_(big[3:3 + B])))   # a slice: offset base
    for off in (1, 5, 16):                               # a base that is 1 / 5 / 16 bytes into an allocation
        flat = torch.zeros(B * H * W + 64, dtype=torch.uint8, device="cuda")
        view = flat[off:off + B * H * W].view(B, H, W)
        view.copy_(torch.as_tensor(masks.view(np.uint8), device="cuda"))
        assert view.data_ptr() % 16 == off % 16
        np.testing.assert_array_equal(words(la.pack_mask_bits(view).bits), want, err_msg=f"offset {off}")
    # a plane stride that is not a multiple of 16 bytes
    flat = torch.zeros(B * (H * W + 3), dtype=torch.uint8, device="cuda")
    view = torch.as_strided(flat, (B, H, W), (H * W + 3, W, 1))
    view.copy_(torch.as_tensor(masks.view(np.uint8), device="cuda"))
    np.testing.assert_array_equal(words(la.pack_mask_bits(view).bits), want, err_msg="odd plane stride")
    # transposed pixels are not dense planes: copied first, same words
    tr = torch.as_tensor(np.ascontiguousarray(masks.transpose(0, 2, 1)).view(np.uint8), device="cuda").transpose(1, 2)
    np.testing.assert_array_equal(words(la.pack_mask_bits(tr).bits), want)


@pytest.mark.parametrize("H,W,pad", [(64, 96, True), (37, 53, True), (37, 53, False)])
def test_pack_into_a_wider_stride_leaves_the_gap_untouched(la, H, W, pad):
    import torch

    rs = np.random.RandomState(6)
    B = 7
    masks = rs.rand(B, H, W) < 0.3
    W_out = padded(W) if pad else W
    want = packbits(masks, W_out)
    nw = want.shape[1]
    for extra in (1, 4, 7):
        out = torch.full((B, nw + extra), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        mb = la.pack_mask_bits(masks, frame_pad=pad, out=out)
        assert mb.bits.data_ptr() == out.data_ptr()
        got = words(out)
        np.testing.assert_array_equal(got[:, :nw], want)
        assert (got[:, nw:] == 0x5A5A5A5A).all(), "the words between two planes were written"
        np.testing.assert_array_equal(np_(la.unpack_mask_bits(mb)), masks)
        np.testing.assert_array_equal(np_(la.mask_stats_bits(mb)), [O.mask_stats(m) for m in masks])
        lo = torch.full((B, nw + extra), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        la.pack_logits_bits(torch.as_tensor(np.where(masks, 1.0, -1.0).astype(np.float32), device="cuda"), frame_pad=pad, out=lo)
        np.testing.assert_array_equal(words(lo), got)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("H,W", [(96, 224), (37, 53)])
def test_pack_logits_bits(la, dtype, H, W):
    import torch

    rs = np.random.RandomState(H + len(dtype))
    B = 6
    x = torch.as_tensor((rs.randn(B, H, W) * 2).astype(np.float32), device="cuda").to(getattr(torch, dtype))
    flat = x.view(-1)
    flat[::17] = float("nan")
    flat[3::29] = float("inf")
    flat[5::31] = float("-inf")
    flat[7::13] = 0.5                                     # values ON a threshold (0.5 is exact in every format): strict >
    flat[11::19] = 0.0
    flat[2::23] = -1.25
    xf = np_(x.float())
    for t in (0.0, 0.5, -1.25):
        with np.errstate(invalid="ignore"):
            want = xf > np.float32(t)                     # NaN compares false
        assert want[np.isposinf(xf)].all() and not want[np.isneginf(xf)].any() and not want[np.isnan(xf)].any()
        np.testing.assert_array_equal(words(la.pack_logits_bits(x, t).bits), packbits(want, padded(W)), err_msg=f"{dtype} t={t}")
        np.testing.assert_array_equal(words(la.pack_logits_bits(x, t, frame_pad=False).bits), packbits(want), err_msg=f"{dtype} t={t} raw")
        # strided planes (every second one) and a base that is one element into an allocation
        big = torch.zeros((2 * B, H, W), dtype=x.dtype, device="cuda")
        big[::2] = x
        np.testing.assert_array_equal(words(la.pack_logits_bits(big[::2], t, frame_pad=False).bits), packbits(want))
        off = torch.zeros(B * H * W + 8, dtype=x.dtype, device="cuda")
        v = off[1:1 + B * H * W].view(B, H, W)
        v.copy_(x)
        np.testing.assert_array_equal(words(la.pack_logits_bits(v, t, frame_pad=False).bits), packbits(want))


@pytest.mark.parametrize("H,W", [(480, 640), (37, 53), (64, 96), (100, 214)])
def test_mask_stats_bits(la, H, W):
    masks = zoo(np.random.RandomState(H + W), H, W)
    want = np.array([O.mask_stats(m) for m in masks])
    for pad in (True, False):
        np.testing.assert_array_equal(np_(la.mask_stats_bits(host_bits(masks, pad))), want, err_msg=f"pad={pad}")
    want3 = np.array([O.mask_stats(m, 3) for m in masks])
    np.testing.assert_array_equal(np_(la.mask_stats_bits(la.pack_mask_bits(masks), boundary_threshold=3)), want3)


# ------------------------------------------------------------------------------------------
# 5. the fit: 480x640, B = 24, against the oracle, the run-length entry and the pinned u8 entry
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grounded", [False, True])
def test_fit_bits_640x480(la, grounded):
    B, H, W = 24, 480, 640
    depth, masks, ground = rle_masks(B, H, W)
    g = ground if grounded else None
    got = la.fit_instances_bits(depth, host_bits(masks), K640, ground=g)
    status = check_oracle(got, depth, masks, K640, f"bits grounded={grounded}", ground=g)
    assert status[B - 1] == 1 and (status == 0).sum() == B - 1
    same_engine(got, rle_on_instance_engine(la, depth, masks, K640, ground=g), "vs run lengths")
    same_engine(got, u8_on_instance_engine(la, depth, masks, K640, ground=g), "vs u8 planes")
    same_engine(got, la.fit_instances_bits(depth, la.pack_mask_bits(masks), K640, ground=g), "host-packed vs device-packed planes")


# ------------------------------------------------------------------------------------------
# 6. batch sizes around the other engines' limits and the launch-order range; the order is invisible
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7, 300, 1100])
def test_batch_sizes_and_launch_order(la, B, monkeypatch):
    import torch

    H, W = 96, 224
    rs = np.random.RandomState(B)
    depth = rs.uniform(0.5, 10, (B, H, W)).astype(np.float32)
    masks = np.zeros((B, H, W), bool)
    for i in range(B):
        h, w = rs.randint(1, H + 1), rs.randint(1, W + 1)
        r0, c0 = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
        masks[i, r0:r0 + h, c0:c0 + w] = True
    if B > 5:
        masks[5] = False
    bits = host_bits(masks)
    d = torch.as_tensor(depth, device="cuda")
    area = masks.reshape(B, -1).sum(1).astype(np.int32)
    ground = np.array([[0.02, -0.98, 0.1, 1.5]] * B) + 0.03 * rs.randn(B, 4)
    for g in (None, ground):
        outs = {}
        for name, order, hint in (("off", False, None), ("on", True, None), ("hint", True, area), ("wrong hint", True, area[::-1].copy()),
                                  ("default", None, None)):
            monkeypatch.setattr(SCHED(), "launch_order", order)
            outs[name] = [np_(t) for t in la.fit_instances_bits(d, bits, K224, ground=g, area_hint=hint)]
        monkeypatch.setattr(SCHED(), "launch_order", None)
        for name in ("on", "hint", "wrong hint", "default"):
            for x, y in zip(outs["off"], outs[name]):
                np.testing.assert_array_equal(x, y, err_msg=f"B={B} launch order {name} changed a record")
        same_engine(outs["off"], rle_on_instance_engine(la, d, masks, K224, ground=g), f"B={B} vs run lengths")
        if B <= 7:
            check_oracle(outs["off"], depth, masks, K224, f"B={B}", ground=g)
        else:
            sel = np.r_[0:12, B - 12:B]
            b, s, a = (x[sel] for x in outs["off"])
            ref, st, nv = oracle(depth[sel], masks[sel], K224, ground=None if g is None else g[sel])
            np.testing.assert_array_equal(s, st)
            assert_records(b[st == 0], ref[st == 0], f"B={B}", gap=a[st == 0, 3])
            assert outs["off"][1][5] == 1 and np.isnan(outs["off"][0][5]).all()


def test_launch_order_keys_are_the_exact_popcount(la, monkeypatch):
    """the order is decided from keys in the workspace: area (18 bits) << 14 | 16383 - instance, the area an exact popcount"""
    import torch

    from labelany3d_amd import InstanceFitter

    B, H, W = 600, 96, 224
    rs = np.random.RandomState(3)
    masks = rs.rand(B, H, W) < rs.uniform(0.0, 0.9, (B, 1, 1))
    bits = host_bits(masks)
    d = torch.as_tensor(rs.uniform(0.5, 10, (B, H, W)).astype(np.float32), device="cuda")
    k = torch.as_tensor(K224, device="cuda")
    monkeypatch.setattr(SCHED(), "launch_order", True)
    f = InstanceFitter(B, H, W, torch.device("cuda", 0))
    f.workspace.zero_()
    f.boxes.fill_(12345.0); f.status.fill_(-1)
    b, s, a = f.run_bits(d, bits, k)
    torch.cuda.synchronize()
    assert int((s < 0).sum()) == 0 and not bool((b == 12345.0).any())
    keys = f.workspace[0][: 4 * B].view(torch.int32).cpu().numpy().astype(np.int64)
    assert ((keys & 16383) == 16383 - np.arange(B)).all()
    np.testing.assert_array_equal(keys >> 14, masks.reshape(B, -1).sum(1))


# ------------------------------------------------------------------------------------------
# 7. frames outside the tiled path, tail bits, the general (4-byte aligned) form
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(37, 53), (100, 214)])
@pytest.mark.parametrize("grounded", [False, True])
def test_frames_outside_the_tiled_path(la, H, W, grounded):
    import torch

    B = 10
    depth, masks, ground = rle_masks(B, H, W, seed=H)
    g = ground if grounded else None
    want_rle = rle_on_instance_engine(la, depth, masks, K224, ground=g)   # (the wrapper pads the depth rows: the tiled form)
    # unpadded rows: the row-linear form (no other entry takes it through the wrappers: against the oracle)
    raw = host_bits(masks, pad=False)
    got = la.fit_instances_bits(depth, raw, K224, ground=g)
    check_oracle(got, depth, masks, K224, f"{W}x{H} unpadded", ground=g)
    # the same frame with rows padded to a multiple of 32 (frame_width): depth padded by the wrapper, and by the caller
    pad = host_bits(masks, pad=True)
    got_p = la.fit_instances_bits(depth, pad, K224, ground=g)
    check_oracle(got_p, depth, masks, K224, f"{W}x{H} padded", ground=g)
    same_engine(got_p, want_rle, "padded vs run lengths")
    dp, fw = la.pad_depth_rows(depth)
    assert fw == W
    same_engine(got_p, la.fit_instances_bits(dp, pad, K224, ground=g, frame_width=W), "caller-padded depth")
    with pytest.raises(ValueError, match="frame_width"):
        la.fit_instances_bits(dp, pad, K224, frame_width=W + 1)
    if (H * W) % 32:
        # ones past H*W in the last word must be ignored
        t = raw[0].clone()
        t[:, -1] |= torch.tensor(np.array(~np.uint32((1 << ((H * W) % 32)) - 1)).view(np.int32).item(), dtype=torch.int32, device="cuda")
        assert (words(t)[:, -1] >> ((H * W) % 32)).all()
        for a, b in zip(got, la.fit_instances_bits(depth, (t, H, W, W), K224, ground=g)):
            np.testing.assert_array_equal(np_(a), np_(b), err_msg="garbage past H*W changed a record")
        np.testing.assert_array_equal(np_(la.mask_stats_bits((t, H, W, W))), [O.mask_stats(m) for m in masks])
        np.testing.assert_array_equal(np_(la.unpack_mask_bits((t, H, W, W))), masks)


@pytest.mark.parametrize("H,W", [(96, 224), (37, 53)])
def test_general_form_equals_the_aligned_call(la, H, W):
    """bits_plane_stride not a multiple of 4 and a base that is only 4-byte aligned: the word form of phase 0"""
    import torch

    B = 9
    depth, masks, ground = rle_masks(B, H, W, seed=W)
    bits = host_bits(masks, pad=False)
    nw = bits[0].shape[1]
    want = la.fit_instances_bits(depth, bits, K224, ground=ground)
    for extra, off in ((0, 1), (1, 0), (3, 3), (5, 2)):
        flat = torch.full((off + B * (nw + extra) + 8,), 0x77777777, dtype=torch.int32, device="cuda")
        view = torch.as_strided(flat, (B, nw), (nw + extra, 1), off)
        view.copy_(bits[0])
        if off:
            assert view.data_ptr() % 16 != 0
        got = la.fit_instances_bits(depth, (view, H, W, W), K224, ground=ground)
        for a, b in zip(want, got):
            np.testing.assert_array_equal(np_(a), np_(b), err_msg=f"stride +{extra}, base +{off} words")
        np.testing.assert_array_equal(np_(la.mask_stats_bits((view, H, W, W))), [O.mask_stats(m) for m in masks])
        np.testing.assert_array_equal(np_(la.unpack_mask_bits((view, H, W, W))), masks)
        sidx = la.draw_sample_idx(masks.reshape(B, -1).sum(1), np.random.RandomState(1))
        for a, b in zip(la.fit_instances_bits(depth, bits, K224, sample_idx=sidx), la.fit_instances_bits(depth, (view, H, W, W), K224, sample_idx=sidx)):
            np.testing.assert_array_equal(np_(a), np_(b))


# ------------------------------------------------------------------------------------------
# 8. shared depth planes, per-image K, 2-D boxes, non-finite and negative depths
# ------------------------------------------------------------------------------------------
def test_image_index_per_image_K_and_boxes2d(la):
    B, P, H, W = 20, 3, 96, 224
    depth, masks, ground = rle_masks(B, H, W, seed=9)
    depth = depth[:P]
    Ks = np.stack([K224, K224 * [[1.1], [0.9], [1]], K224 * [[0.9], [1.2], [1]]])
    Ks[2, 0, 1] = 2.5                                             # a skewed camera: the two-pass form
    ii = (np.arange(B) % P).astype(np.int32)
    for g in (None, ground):
        got = la.fit_instances_bits(depth, host_bits(masks), Ks, ground=g, image_index=ii, image_size=(W, H))
        assert len(got) == 4
        check_oracle(got, depth, masks, Ks, "image_index", ground=g, depth_index=ii)
        boxes, status, b2 = np_(got[0]), np_(got[1]), np_(got[3])
        for n in range(B):
            if status[n] == 0:
                np.testing.assert_allclose(b2[n], np.ravel(O.project_boxes(boxes[n:n + 1], Ks[ii[n]], (W, H))), rtol=1e-9, atol=1e-9)
            else:
                assert np.isnan(b2[n]).all()
        same_engine(got, rle_on_instance_engine(la, depth, masks, Ks, ground=g, image_index=ii), "vs run lengths")
    with pytest.raises(ValueError, match="image_index"):
        la.fit_instances_bits(depth, host_bits(masks), Ks, image_index=np.full(B, P, np.int32))


def test_nonfinite_and_negative_depths_under_the_mask(la):
    B, H, W = 10, 96, 224
    depth, masks, ground = rle_masks(B, H, W, seed=11)
    depth[4][masks[4]] = np.nan                                   # all NaN: status 1
    r, c = np.argwhere(masks[5])[10]
    depth[5, r, c] = np.inf                                       # an inf under the mask
    r, c = np.argwhere(masks[6])[20]
    depth[6, r, c] = np.nan                                       # a NaN hole: dropped
    r, c = np.argwhere(masks[3])[7]
    depth[3, r, c] = -2.0                                         # a negative depth: fitted
    for g in (None, ground):
        got = la.fit_instances_bits(depth, host_bits(masks), K224, ground=g)
        status = check_oracle(got, depth, masks, K224, "nonfinite", ground=g)
        u8 = u8_on_instance_engine(la, depth, masks, K224, ground=g)
        same_engine(got, u8, "vs u8 planes")
        # (an infinite depth under the mask is dropped like a NaN by the oracle and by the u8 call alike: float32 depths never
        # carry an infinite coordinate into the PCA, so status 4 does not arise on this path; whatever the u8 call reports is asserted above)
        assert status[4] == 1 and status[5] == np_(u8[1])[5] == 0 and status[6] == 0 and status[3] == 0 and status[B - 1] == 1
        assert np_(got[2])[5, 1] == masks[5].sum() - 1
        assert np_(got[2])[6, 1] == masks[6].sum() - 1


# ------------------------------------------------------------------------------------------
# 9. reference-subsample mode
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["no_ground", "ground", "skewed_K"])
@pytest.mark.parametrize("H,W", [(96, 224), (100, 214), (480, 640)])
def test_subsample_mode(la, case, H, W):
    B = 16
    depth, masks, ground = rle_masks(B, H, W, seed=13 + H)
    for n in (2, 9):                                              # masks of at most 500 pixels: not sampled
        masks[n] = False
        masks[n, 30:30 + 12 + n, 40:60] = True
    K = (K640 if W == 640 else K224).copy()
    g = None
    if case == "ground":
        g = ground.copy()
        g[::4, 0] = np.nan
    if case == "skewed_K":
        K[0, 1] = 3.0
    counts = masks.reshape(B, -1).sum(1)
    assert (counts[[2, 9]] <= 500).all() and (counts > 500).sum() >= B // 2
    sidx = la.draw_sample_idx(counts, np.random.RandomState(17))
    got = la.fit_instances_bits(depth, host_bits(masks), K, ground=g, sample_idx=sidx)
    check_oracle(got, depth, masks, K, f"subsample {case}", ground=g, sample_idx=sidx)
    same_engine(got, rle_on_instance_engine(la, depth, masks, K, ground=g, sample_idx=sidx), "vs run lengths")


# ------------------------------------------------------------------------------------------
# 10. convex-hull yaw
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(7, 96, 224), (300, 96, 224), (40, 480, 640)])
def test_hull_full_mask(la, B, H, W):
    depth, masks, K = hull_scene(200 + B, B, H, W)
    got = la.fit_instances_bits(depth, host_bits(masks), K, method="convex_hull")
    check_hull_against_oracle(got, depth, masks, K, f"bits hull B={B} {W}x{H}")
    for a, b in zip(got, la.fit_instances(depth, masks, K, method="convex_hull")):
        np.testing.assert_array_equal(np_(a), np_(b), err_msg="bit planes differ from u8 planes")


def test_hull_padded_width(la):
    depth, masks, K = hull_scene(8, 12, 96, 214)
    got = la.fit_instances_bits(depth, host_bits(masks), K, method="convex_hull")
    check_hull_against_oracle(got, depth, masks, K, "bits hull W=214")
    for a, b in zip(got, la.fit_instances_rle(depth, [O.rle_encode(m) for m in masks], K, method="convex_hull")):
        np.testing.assert_array_equal(np_(a), np_(b))


def test_hull_subsample_mode_with_ground(la):
    B, H, W = 40, 96, 224
    depth, masks, K = hull_scene(13, B, H, W)
    for n in (2, 9):
        masks[n] = False
        masks[n, 30:30 + 12 + n, 40:60] = True
    rs = np.random.RandomState(3)
    ground = np.array([[0.02, -0.98, 0.1, 1.5]] * B) + 0.03 * rs.randn(B, 4)
    ground[::4, 0] = np.nan
    sidx = la.draw_sample_idx(masks.reshape(B, -1).sum(1), np.random.RandomState(17))
    got = la.fit_instances_bits(depth, host_bits(masks), K, ground=ground, sample_idx=sidx, method="convex_hull")
    check_hull_against_oracle(got, depth, masks, K, "bits hull subsample", ground=ground, sample_idx=sidx)
    for a, b in zip(got, la.fit_instances(depth, masks, K, ground=ground, sample_idx=sidx, method="convex_hull")):
        np.testing.assert_array_equal(np_(a), np_(b))


def test_hull_refusals_are_the_u8_call_s(la):
    B, H, W = 16, 96, 224
    depth, masks, K = hull_scene(14, B, H, W)
    ground = np.full((B, 4), np.nan)
    grounded = np.zeros(B, bool)
    grounded[[1, 6, 7, 13]] = True
    ground[grounded] = [0.02, -0.98, 0.1, 1.5]
    masks[10] = True                                              # a whole-frame mask: no room for the column arrays
    grounded[10] = True
    bits = host_bits(masks)
    got = [np_(t) for t in la.fit_instances_bits(depth, bits, K, ground=ground, method="convex_hull")]
    assert (got[1][grounded] == 5).all() and np.isnan(got[0][grounded]).all() and (got[1][~grounded] != 5).all()
    for a, b in zip(got, la.fit_instances(depth, masks, K, ground=ground, method="convex_hull")):
        np.testing.assert_array_equal(a, np_(b))
    Ks = np.stack([K] * B)
    skew = np.zeros(B, bool)
    skew[[0, 5, 10, 11]] = True
    Ks[skew, 0, 1] = 2.0
    got = [np_(t) for t in la.fit_instances_bits(depth, bits, Ks, method="convex_hull")]
    assert (got[1][skew] == 5).all() and np.isnan(got[0][skew]).all() and (got[1][~skew] != 5).all()
    for a, b in zip(got, la.fit_instances(depth, masks, Ks, method="convex_hull")):
        np.testing.assert_array_equal(a, np_(b))
    # a frame outside the tiled path in full-mask mode: every instance refused, as the u8 call refuses it
    d2, m2, K2 = hull_scene(15, 5, 37, 53)
    got = [np_(t) for t in la.fit_instances_bits(d2, host_bits(m2, pad=False), K2, method="convex_hull")]
    assert (got[1] == 5).all() and np.isnan(got[0]).all()


# ------------------------------------------------------------------------------------------
# 11. the fused filter, both height rules
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(96, 224), (100, 214)])
def test_fused_filter_both_height_rules(la, H, W):
    B = 24
    rs = np.random.RandomState(21)
    depth = rs.uniform(0.5, 10, (B, H, W)).astype(np.float32)
    masks = np.zeros((B, H, W), bool)
    for i in range(B):                                            # rectangles clear of the 10-px border strips
        h, w = rs.randint(8, H - 24), rs.randint(12, W - 24)
        r0, c0 = rs.randint(11, H - 11 - h + 1), rs.randint(11, W - 11 - w + 1)
        masks[i, r0:r0 + h, c0:c0 + w] = True
    masks[3] = False; masks[3, 40:44, 50:54] = True               # below min_area
    masks[5] = False; masks[5, 0:60, 0:40] = True                 # touches the border
    masks[7] = False; masks[7, 20:23, 40:60] = True; masks[7, 60:63, 40:60] = True   # six rows holding pixels, a span of 43
    masks[8] = False; masks[8, 15:18, 30:80] = True               # three rows: too low by both rules
    masks[9] = False                                              # empty
    masks[11] = False; masks[11, 12:H - 12, W - 14:W - 11] = True  # three columns next to the right strip of the UNPADDED frame
    masks[12] = False; masks[12, 12:H - 12, W - 12:W - 9] = True   # ... and reaching into it
    bits = host_bits(masks)
    stats_want = np.array([O.mask_stats(m) for m in masks])
    plain = [np_(t) for t in la.fit_instances_bits(depth, bits, K224)]
    kept_by = {}
    for rule, from_rle in (("rows", True), ("span", False)):
        fb, fs, fa, st = (np_(t) for t in la.fit_instances_bits(depth, bits, K224, filter=True, height_rule=rule))
        np.testing.assert_array_equal(st, stats_want, err_msg=f"{rule}: statistics")
        keep = np.array([O.keep_instance(s, H, from_rle) for s in stats_want])
        np.testing.assert_array_equal(fs == 6, ~keep, err_msg=f"{rule}: kept set")
        assert np.isnan(fb[~keep]).all()
        np.testing.assert_array_equal(fb[keep], plain[0][keep])
        np.testing.assert_array_equal(fs[keep], plain[1][keep])
        np.testing.assert_array_equal(fa[keep], plain[2][keep])
        kept_by[rule] = keep
        # the thresholds of the dict form
        fb2, fs2, _, st2 = (np_(t) for t in la.fit_instances_bits(depth, bits, K224, filter={"boundary_threshold": 3, "scale_threshold": 10},
                                                                   height_rule=rule))
        want2 = np.array([O.mask_stats(m, 3) for m in masks])
        np.testing.assert_array_equal(st2, want2)
        np.testing.assert_array_equal(fs2 == 6, ~np.array([O.keep_instance(s, H, from_rle, 10) for s in want2]))
    assert not kept_by["rows"][7] and kept_by["span"][7] and not kept_by["span"][8]
    assert kept_by["rows"][11] and not kept_by["rows"][12] and kept_by["rows"].sum() >= B // 2
    # the run-length entry's filter is the "rows" rule
    rb, rs_, ra, rst = rle_on_instance_engine(la, depth, masks, K224, filter=True)
    got = la.fit_instances_bits(depth, bits, K224, filter=True)
    same_engine(got, (rb, rs_, ra), "filtered vs run lengths")
    np.testing.assert_array_equal(np_(got[3]), np_(rst))
    with pytest.raises(ValueError, match="height_rule"):
        la.fit_instances_bits(depth, bits, K224, filter=True, height_rule="both")


# ------------------------------------------------------------------------------------------
# 12. pins give way; builds
# ------------------------------------------------------------------------------------------
def test_pinned_engines_and_builds(la, monkeypatch):
    B, H, W = 12, 96, 224
    depth, masks, ground = rle_masks(B, H, W, seed=15)
    bits = host_bits(masks)
    for g in (None, ground):
        want = [np_(t) for t in la.fit_instances_bits(depth, bits, K224, ground=g)]
        assert (want[1][:B - 1] == 0).all()
        for engine in ("rows", "rows2", "band", "split", "instance"):
            monkeypatch.setattr(SCHED(), "engine", engine)
            got = [np_(t) for t in la.fit_instances_bits(depth, bits, K224, ground=g)]
            for a, b in zip(want, got):
                np.testing.assert_array_equal(a, b, err_msg=f"pinned {engine}")
        monkeypatch.setattr(SCHED(), "engine", None)
        for build in ("plain", "nocull"):
            monkeypatch.setattr(SCHED(), "build", build)
            got = [np_(t) for t in la.fit_instances_bits(depth, bits, K224, ground=g)]
            same_engine(got, rle_on_instance_engine(la, depth, masks, K224, ground=g), f"build {build} vs run lengths")
            monkeypatch.setattr(SCHED(), "build", None)
            np.testing.assert_array_equal(got[1], want[1])
            np.testing.assert_array_equal(got[2][:, 1:3], want[2][:, 1:3])
            # (the default un-grounded call takes the separable single pass: equal to rounding - the bound of tests/test_gpu_shard.py)
            np.testing.assert_allclose(np.nan_to_num(got[0][:, :15], nan=-7.0), np.nan_to_num(want[0][:, :15], nan=-7.0), rtol=1e-11, atol=1e-11)
            check_oracle(got, depth, masks, K224, f"build {build}", ground=g)


# ------------------------------------------------------------------------------------------
# 13. run_bits captured into a graph
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["pca", "convex_hull"])
def test_run_bits_captured_into_a_graph(la, method):
    """one launch (two for a hull call) in a linear chain on one stream: captured once, replayed on fresh inputs"""
    import torch

    from labelany3d_amd import InstanceFitter

    B, H, W = 300, 96, 224                                        # (inside the launch-order range: the captured call keeps the helper kernel)
    dev = torch.device("cuda", 0)
    depth0, masks0, K = hull_scene(17, B, H, W)
    d = torch.as_tensor(depth0, device=dev)
    m = host_bits(masks0)[0]
    k = torch.as_tensor(K, device=dev)
    f = InstanceFitter(B, H, W, dev, method=method)
    side = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        f.run_bits(d, m, k, stream=side)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            f.run_bits(d, m, k, stream=torch.cuda.current_stream())
    fr = InstanceFitter(B, H, W, dev, method=method)
    for seed in (18, 19):
        depth1, masks1, _ = hull_scene(seed, B, H, W)
        d.copy_(torch.as_tensor(depth1, device=dev)); m.copy_(host_bits(masks1)[0])
        f.boxes.fill_(12345.0); f.status.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        rb, rs_, ra = fr.run_bits(d, m, k)
        torch.cuda.synchronize()
        assert torch.equal(f.status[0], rs_) and (rs_ == 0).all()
        assert torch.equal(f.boxes[0], rb) and torch.equal(f.aux[0], ra)
        ub, us, ua = fr.run(d, torch.as_tensor(masks1.view(np.uint8), device=dev), k, engine="instance")
        torch.cuda.synchronize()
        same_engine((rb, rs_, ra), (ub, us, ua), "run_bits vs run")
    if method == "pca":
        with pytest.raises(ValueError, match="sized for method='pca'"):
            f.run_bits(d, m, k, method="convex_hull")
    with pytest.raises(ValueError, match="bit planes"):
        f.run_bits(d, m[:, :-1], k)


# ------------------------------------------------------------------------------------------
# 14. seeded randomised sweep
# ------------------------------------------------------------------------------------------
SWEEP_FRAMES = [(8, 32), (16, 32), (24, 48), (37, 53), (64, 96), (96, 128), (96, 224), (100, 214), (128, 427), (160, 320), (333, 500),
                (480, 640), (517, 672)]


def _sweep_case(rs):
    H, W = SWEEP_FRAMES[rs.randint(len(SWEEP_FRAMES))]
    px = H * W
    bmax = 300 if px <= 8192 else 40 if px <= 32768 else 12 if px <= 131072 else 5
    B = int(rs.randint(1, bmax + 1)) if rs.rand() < 0.5 else int(rs.randint(1, min(bmax, 12) + 1))
    shared = B > 1 and rs.rand() < 0.4
    P = int(rs.randint(1, min(B, 4) + 1)) if shared else B
    depth_kind = rs.randint(3)
    if depth_kind == 0:
        depth = rs.uniform(0.3, 12, (P, H, W)).astype(np.float32)
    else:
        vv, uu = np.mgrid[0:H, 0:W]
        depth = (2 + 0.01 * uu[None] + 0.02 * vv[None] + rs.uniform(0, 3, (P, 1, 1)) + (0.05 * rs.randn(P, H, W) if depth_kind == 2 else 0)).astype(np.float32)
    masks = np.zeros((B, H, W), bool)
    for i in range(B):
        kind = rs.choice(5, p=[0.4, 0.2, 0.3, 0.05, 0.05])
        if kind == 0:
            h, w = rs.randint(1, H + 1), rs.randint(1, W + 1)
            r0, c0 = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
            masks[i, r0:r0 + h, c0:c0 + w] = True
        elif kind == 1:
            masks[i] = rs.rand(H, W) < rs.uniform(0.005, 0.7)
        elif kind == 2:
            vv, uu = np.mgrid[0:H, 0:W]
            masks[i] = ((vv - rs.uniform(0, H)) / rs.uniform(1, H)) ** 2 + ((uu - rs.uniform(0, W)) / rs.uniform(1, W)) ** 2 < 1
        elif kind == 3:
            masks[i, rs.randint(0, H), rs.randint(0, W)] = True   # a single pixel: too few points
        # kind 4: empty
    if rs.rand() < 0.25:
        for _ in range(rs.randint(1, 5)):
            depth[rs.randint(0, P), rs.randint(0, H), rs.randint(0, W)] = rs.choice([np.nan, np.inf, -np.inf])
    gkind = rs.randint(3)                                         # ground for none / all / some (NaN rows)
    ground = None
    if gkind:
        ground = np.array([[0.02, -0.98, 0.1, 1.5]] * B) + 0.05 * rs.randn(B, 4)
        if gkind == 2:
            ground[rs.rand(B) < 0.5, 0] = np.nan
    K = np.array([[rs.uniform(40, 600), 0, W / 2 + rs.uniform(-5, 5)], [0, rs.uniform(40, 600), H / 2 + rs.uniform(-5, 5)], [0, 0, 1]])
    if rs.rand() < 0.15:
        K[0, 1] = rs.uniform(-3, 3)
    ii = rs.randint(0, P, B).astype(np.int32) if shared else None
    sample = rs.rand() < 0.35
    return depth, masks, K, ground, ii, sample


@pytest.mark.parametrize("chunk", range(5))
def test_randomised_sweep(la, chunk):
    """5 x 32 = 160 seeded cases, none skipped: bit planes vs the oracle and vs the run-length entry"""
    rs = np.random.RandomState(4000 + chunk)
    n_ok = n_all = 0
    for case in range(32):
        depth, masks, K, ground, ii, sample = _sweep_case(rs)
        B, H, W = masks.shape
        sidx = la.draw_sample_idx(masks.reshape(B, -1).sum(1), rs) if sample else None
        tag = f"chunk {chunk} case {case}: B={B} {W}x{H} planes={len(depth)} ground={ground is not None} sample={sample}"
        got = la.fit_instances_bits(depth, host_bits(masks), K, ground=ground, image_index=ii, sample_idx=sidx)
        status = check_oracle(got, depth, masks, K, tag, ground=ground, sample_idx=sidx, depth_index=ii)
        same_engine(got, rle_on_instance_engine(la, depth, masks, K, ground=ground, image_index=ii, sample_idx=sidx), tag + " vs run lengths")
        n_ok += int((status == 0).sum()); n_all += B
    print(f"sweep chunk {chunk}: {n_ok} of {n_all} instances fitted (status 0)")
    assert 2 * n_ok >= n_all
