"""CPU-only contract of the instance point clouds (include/la3d.h "instance point clouds": ``la3d_instance_point_offsets``,
``la3d_gather_instance_points``): the exports exist on every layer, the new argument block has its pinned size and the old ones
keep theirs, the C entries refuse before any launch, the Python argument errors come before any device work, and the NumPy
restatement the GPU tests compare with (tests/instance_points_cases.py) is ``pts[mask]`` of the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import la3d_oracle as O

from . import instance_points_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_C = ("la3d_instance_points_workspace_bytes", "la3d_instance_point_offsets", "la3d_gather_instance_points")
NEW_PY = ("instance_points", "instance_points_frames", "InstancePoints")


def test_exports_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    for fn in NEW_C:
        assert re.search(rf"\b{fn}\s*\(", hdr), fn
        assert fn in _lib.EXPORTS and hasattr(_lib.lib, fn), fn
    for fn in NEW_PY:
        assert callable(getattr(la, fn)) and fn in la.__all__, fn
    for name, val in (("LA3D_CLOUD_OK", 0), ("LA3D_CLOUD_NO_ROOM", 1), ("LA3D_CLOUD_MISMATCH", 2)):
        assert re.search(rf"#define {name} {val}\b", hdr), name
    assert (_lib.CLOUD_OK, _lib.CLOUD_NO_ROOM, _lib.CLOUD_MISMATCH) == (0, 1, 2)
    assert "instance point clouds" in hdr


def test_additive_abi_and_pinned_block_size():
    from labelany3d_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2
    assert C.sizeof(_lib.FitArgs) == 232 and C.sizeof(_lib.Depth16Block) == 32 and C.sizeof(_lib.Frame) == 24
    assert C.sizeof(_lib.CloudArgs) == 192
    assert _lib.CloudArgs._fields_[0][0] == "struct_size" and _lib.CloudArgs._fields_[-1][0] == "stream"
    # the field order of the header
    body = re.search(r"typedef struct la3d_cloud_args \{(.*?)\} la3d_cloud_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.CloudArgs._fields_]


def test_workspace_size():
    from labelany3d_amd import _lib

    ws = _lib.lib.la3d_instance_points_workspace_bytes
    assert ws(0, 480, 640) == 0 and ws(4, 0, 640) == 0 and ws(4, 480, 0) == 0
    for B, H, W in ((1, 480, 640), (16, 480, 640), (256, 480, 640), (1024, 480, 640), (7, 33, 47), (100000, 5, 13)):
        n = ws(B, H, W)
        assert n % 4 == 0 and n >= B * 2 * 4          # at least one band count and the total per instance
        assert n <= B * 4 * (max(64, -(-H * ((W + 31) // 32 * 32) // 65536)) + 1)
    assert ws(1, 480, 640) > ws(1, 8, 640)            # a small batch is split into bands of rows


def _block(**kw):
    from labelany3d_amd import _lib

    buf = (C.c_double * 64)()                          # fake "device" memory: every call below is refused before any launch
    p = C.addressof(buf)
    a = _lib.CloudArgs(struct_size=C.sizeof(_lib.CloudArgs), B=2, H=8, W=32, depth=p, mask=p, K=p, counts=p, offsets=p, points=p,
                       status=p, workspace=p, capacity=16)
    for k, v in kw.items():
        setattr(a, k, v)
    a._keep = buf
    return a, p


def _d16(**kw):
    from labelany3d_amd import _lib

    buf = (C.c_uint16 * 8)()
    d = dict(struct_size=C.sizeof(_lib.Depth16Block), dtype=_lib.DTYPE_U16, planes=C.addressof(buf), plane_stride=0, scale=0.001, flags=0)
    d.update(kw)
    blk = _lib.Depth16Block(**d)
    blk._keep = buf
    return blk


REFUSALS = [
    ("struct_size", dict(struct_size=100), -1, "struct_size"),
    ("mask and mask_bits", dict(mask_bits="p"), -1, "mask / mask_bits"),
    ("no mask", dict(mask=None), -1, "mask / mask_bits"),
    ("no depth", dict(depth=None), -1, "depth / depth16"),
    ("frame_width > W", dict(frame_width=33), -1, "frame_width"),
    ("frame_width < 0", dict(frame_width=-1), -1, "frame_width"),
    ("negative B", dict(B=-1), -1, "sizes"),
    ("negative H", dict(H=-1), -1, "sizes"),
    ("negative W", dict(W=-2, frame_width=0), -1, "sizes"),
    ("empty frame", dict(H=0), -1, "sizes"),
    ("offsets NULL", dict(offsets=None), -1, "offsets"),
    ("K NULL", dict(K=None), -1, "K is NULL"),
    ("workspace NULL", dict(workspace=None), -1, "workspace"),
    ("misaligned mask_bits", dict(mask=None, mask_bits="p+2"), -1, "mask_bits"),
    ("mask stride", dict(mask_plane_stride=255), -1, "mask_plane_stride"),
    ("k_stride", dict(k_stride=5), -1, "k_stride"),
    ("frames with u8 masks", dict(frames="p", P=1, image_index="p"), -1, "u8 masks"),
    ("misaligned frames", dict(mask=None, mask_bits="p", frames="p+4", P=1, image_index="p", bits_offsets="p"), -1, "frames"),
    ("misaligned bits_offsets", dict(mask=None, mask_bits="p", frames="p", P=1, image_index="p", bits_offsets="p+4"), -1, "bits_offsets"),
    ("frames mask_bits 16-byte", dict(mask=None, mask_bits="p+4", frames="p", P=1, image_index="p", bits_offsets="p"), -1, "16-byte"),
    ("frames without image_index", dict(mask=None, mask_bits="p", frames="p", P=1, bits_offsets="p"), -1, "image_index"),
    ("frames with frame_width", dict(mask=None, mask_bits="p", frames="p", P=1, image_index="p", bits_offsets="p", frame_width=16), -1, "frames call"),
    ("bits_offsets without frames", dict(mask=None, mask_bits="p", bits_offsets="p"), -1, "bits_offsets"),
    ("W beyond a band", dict(W=65537), -2, "65536"),
    ("H * W beyond int32", dict(H=40000, W=60000), -2, "2^31"),
]


@pytest.mark.parametrize("entry", ["la3d_instance_point_offsets", "la3d_gather_instance_points"])
@pytest.mark.parametrize("name,kw,code,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_c_entries_refuse_before_any_launch(entry, name, kw, code, msg):
    from labelany3d_amd import _lib

    a, p = _block()
    for k, v in kw.items():
        if isinstance(v, str):
            v = p + (int(v[2:]) if len(v) > 1 else 0)
        setattr(a, k, v)
    assert getattr(_lib.lib, entry)(C.byref(a)) == code, name
    assert msg.encode() in _lib.lib.la3d_last_error(), (name, _lib.lib.la3d_last_error())
    assert entry.encode() in _lib.lib.la3d_last_error()


def test_stage_specific_and_depth16_refusals():
    from labelany3d_amd import _lib

    lib = _lib.lib
    assert lib.la3d_instance_point_offsets(None) == -1 and lib.la3d_gather_instance_points(None) == -1
    a, _ = _block(counts=None)
    assert lib.la3d_instance_point_offsets(C.byref(a)) == -1 and b"counts" in lib.la3d_last_error()
    for kw in (dict(points=None), dict(status=None)):
        a, _ = _block(**kw)
        assert lib.la3d_gather_instance_points(C.byref(a)) == -1 and b"points / status" in lib.la3d_last_error()
    a, _ = _block(capacity=-1)
    assert lib.la3d_gather_instance_points(C.byref(a)) == -1 and b"capacity" in lib.la3d_last_error()
    # both depth sources; and every way a la3d_depth16 can be wrong
    blk = _d16()
    a, _ = _block(depth16=C.pointer(blk))
    assert lib.la3d_instance_point_offsets(C.byref(a)) == -1 and b"depth / depth16" in lib.la3d_last_error()
    for bad, msg in ((dict(struct_size=8), b"struct_size of la3d_depth16"), (dict(dtype=_lib.DTYPE_BF16), b"dtype"),
                     (dict(scale=0.0), b"scale"), (dict(scale=float("inf")), b"scale"), (dict(scale=float("nan")), b"scale"),
                     (dict(flags=2), b"flags"), (dict(dtype=_lib.DTYPE_F16, flags=1), b"flags"), (dict(planes=None), b"planes"),
                     (dict(plane_stride=-1), b"stride"), (dict(plane_stride=100), b"stride")):
        blk = _d16(**bad)
        for fn in (lib.la3d_instance_point_offsets, lib.la3d_gather_instance_points):
            a, _ = _block(depth=None, depth16=C.pointer(blk))
            assert fn(C.byref(a)) == -1 and msg in lib.la3d_last_error(), (bad, lib.la3d_last_error())
    blk = _d16()
    a, _ = _block(depth=None, depth16=C.pointer(blk), depth_plane_stride=256)
    assert lib.la3d_gather_instance_points(C.byref(a)) == -1 and b"depth_plane_stride" in lib.la3d_last_error()
    # a frames call takes the flat buffer: no plane stride, an aligned base
    blk = _d16(plane_stride=512)
    a, p = _block(depth=None, depth16=C.pointer(blk), mask=None, mask_bits=1, frames=1, P=1, image_index=1, bits_offsets=1)
    a.mask_bits = a.frames = a.image_index = a.bits_offsets = p
    assert lib.la3d_instance_point_offsets(C.byref(a)) == -1 and b"frames call" in lib.la3d_last_error()
    a, p = _block(mask=None, frames=1, P=1)
    a.mask_bits = a.frames = a.image_index = a.bits_offsets = p
    a.depth = p + 4
    assert lib.la3d_instance_point_offsets(C.byref(a)) == -1 and b"aligned" in lib.la3d_last_error()


def test_python_argument_errors_come_before_device_work(monkeypatch):
    import torch

    from labelany3d_amd import Depth16, FrameBits, instance_points, instance_points_frames, pack_frames

    def no_device(*a, **k):
        raise AssertionError("the entry touched the device before it checked its arguments")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    d, m, K = np.zeros((8, 32), np.float32), np.zeros((2, 8, 32), bool), np.eye(3)
    with pytest.raises(ValueError, match="out_dtype"):
        instance_points(d, m, K, out_dtype=torch.float16)
    for cap in (-1, 2.5, "3", True):
        with pytest.raises(ValueError, match="capacity"):
            instance_points(d, m, K, capacity=cap)
    with pytest.raises(ValueError, match=r"\(B,H,W\)"):
        instance_points(d, m[0], K)
    with pytest.raises(ValueError, match="Depth16 needs"):
        instance_points(Depth16(torch.zeros(8, 32)), m, K)
    with pytest.raises(ValueError, match="scale"):
        instance_points(Depth16(torch.zeros((8, 32), dtype=torch.uint16), scale=0.0), m, K)
    with pytest.raises(ValueError, match=r"\(bits, H, W, frame_width\)"):
        instance_points(d, (torch.zeros(2, 8, dtype=torch.int32), 8, 32), K)
    sizes = [(8, 32), (16, 64)]
    pf = pack_frames([np.ones(s, np.float32) for s in sizes], device="cpu")
    fb = FrameBits(torch.zeros(64, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32),
                   torch.zeros(1, dtype=torch.int32), pf.table_host, pf.H, pf.W)
    with pytest.raises(ValueError, match="PackedFrames"):
        instance_points_frames(np.zeros((8, 32), np.float32), fb, K)
    with pytest.raises(ValueError, match="FrameBits"):
        instance_points_frames(pf, (fb.bits, fb.offsets), K)
    with pytest.raises(ValueError, match="out_dtype"):
        instance_points_frames(pf, fb, K, out_dtype=torch.int32)
    with pytest.raises(ValueError, match="capacity"):
        instance_points_frames(pf, fb, K, capacity=-5)
    other = pack_frames([np.ones((8, 64), np.float32), np.ones((16, 64), np.float32)], device="cpu")
    with pytest.raises(ValueError, match="another frame table"):
        instance_points_frames(other, fb, K)
    with pytest.raises(ValueError, match="live on the GPU"):
        instance_points_frames(pf, fb, K)


def test_numpy_restatement_is_pts_mask_of_the_oracle():
    """33 x 47 with a NaN, an inf, a zero and a negative depth under the masks: counts, offsets, order and pixels; the inf row is NaN
    (0 * inf in the identity rotation), as on the reference."""
    H, W = 33, 47
    depth, masks, K = IC.special_depth(3, H, W), IC.standard_masks(H, W), IC.cameras(3, H, W)
    ii = np.arange(10) % 3
    pts, pix, offsets, counts = IC.cloud_rule(depth, masks, K, ii)
    np.testing.assert_array_equal(counts, masks.reshape(10, -1).sum(1))
    np.testing.assert_array_equal(offsets, np.concatenate([[0], np.cumsum(counts)]))
    assert offsets[0] == offsets[1] == 0 and counts[0] == 0                       # the empty instance
    seen = set()
    for n in range(10):
        full = O.depth_to_points(depth[ii[n]][None], K[ii[n]])
        want = full[masks[n]]
        got = pts[offsets[n]:offsets[n + 1]]
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, full.reshape(-1, 3)[pix[offsets[n]:offsets[n + 1]]])
        np.testing.assert_array_equal(pix[offsets[n]:offsets[n + 1]], np.flatnonzero(masks[n]))
        dn = depth[ii[n]][masks[n]]
        assert np.isnan(got[np.isinf(dn)]).all() and np.isnan(got[np.isnan(dn)]).all()
        zero = got[dn == 0]
        assert (zero == 0).all()
        assert (got[dn < 0][:, 2] < 0).all() or not np.isfinite(dn[dn < 0]).all()
        seen |= {k for k, f in (("nan", np.isnan), ("inf", np.isinf)) if f(dn).any()} | ({"zero"} if (dn == 0).any() else set()) | \
            ({"neg"} if ((dn < 0) & np.isfinite(dn)).any() else set())
    assert seen == {"nan", "inf", "zero", "neg"}


@pytest.mark.parametrize("N", [500, 501])
def test_sample_rule_at_the_threshold(N):
    """the reference's rule (src/util_3dbox.py:123): a cloud of more than 500 points is replaced by its 500 drawn rows, one of exactly
    500 is kept whole"""
    H, W = 33, 47
    depth, K = IC.special_depth(1, H, W), IC.cameras(1, H, W)[0]
    masks = np.zeros((2, H, W), bool)
    masks[0].reshape(-1)[3:3 + N] = True
    masks[1, 4, 5:9] = True
    idx = np.random.RandomState(N).randint(0, N, (2, 500)).astype(np.int32)
    idx[0, 7] = idx[0, 8]                      # a repeated rank
    idx[0, 9], idx[0, 10] = N, -1              # ranks outside the cloud
    pts, pix, offsets, counts = IC.cloud_rule(depth, masks, K, None, idx)
    cloud = O.depth_to_points(depth, K)[masks[0]]
    assert counts.tolist() == [N, 4]
    if N == 500:
        assert offsets.tolist() == [0, 500, 504]
        np.testing.assert_array_equal(pts[:500], cloud)
    else:
        assert offsets.tolist() == [0, 500, 504]
        ok = np.ones(500, bool); ok[[9, 10]] = False
        np.testing.assert_array_equal(pts[:500][ok], cloud[idx[0][ok]])
        np.testing.assert_array_equal(pts[7], pts[8])
        assert np.isnan(pts[[9, 10]]).all() and (pix[[9, 10]] == -1).all()
        np.testing.assert_array_equal(pix[:500][ok], np.flatnonzero(masks[0])[idx[0][ok]])
    np.testing.assert_array_equal(pts[500:], O.depth_to_points(depth, K)[masks[1]])
