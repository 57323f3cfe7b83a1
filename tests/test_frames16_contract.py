"""CPU-only contract of the frames call on 16-bit depth planes (include/la3d.h "images of different sizes in one call":
``la3d_fit_instances_frames_depth16``; ``pack_frames(dtype=...)`` / ``PackedFrames16`` / ``ScenePipeline(depth_dtype=...)``): the
binding with the header's signature, every call-level refusal through the C entry before any launch (host dummies stand in for the
device pointers: a refused call never touches them), the layout of the 16-bit packer on the host, the Python argument errors before
any device work, and the synthetic scene trees in 16-bit dtypes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import depth16_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "la3d_fit_instances_frames_depth16"


def test_binding_has_the_headers_signature():
    from labelany3d_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    m = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, "the header does not declare the entry"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const la3d_fit_args* args", "const la3d_depth16* depth", "const la3d_frame* frames", "int32_t P"]
    assert hasattr(_lib.lib, NAME) and NAME in _lib.EXPORTS
    fn = getattr(_lib.lib, NAME)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.POINTER(_lib.FitArgs), C.POINTER(_lib.Depth16Block), C.c_void_p, C.c_int32]
    # a new symbol only: no struct changes, the ABI version stays
    assert _lib.lib.la3d_version() == 2 and C.sizeof(_lib.FitArgs) == 232 and C.sizeof(_lib.Depth16Block) == 32 and C.sizeof(_lib.Frame) == 24
    assert not re.search(r"la3d_fit_instances_frames, la3d_fit_annotations_host and the positional entries take float32 planes only", hdr)
    # the la3d_frame comment says which unit depth_offset counts in for each entry
    row = hdr[hdr.index("typedef struct la3d_frame"):hdr.index("} la3d_frame;")]
    assert "la3d_fit_instances_frames_depth16" in row and "16-bit" in row and "floats" in row
    import labelany3d_amd as la
    assert "PackedFrames16" in la.__all__
    assert la.PackedFrames16._fields == ("data", "table", "table_host", "H", "W", "sizes", "scale", "zero_is_hole")


def _block(_lib, one, **kw):
    p = C.addressof(one)
    base = dict(struct_size=C.sizeof(_lib.FitArgs), B=1, H=8, W=32, rle_counts=p, rle_offsets=p, K=p, out=p, status=p, workspace=p, image_index=p)
    base.update(kw)
    return _lib.FitArgs(**base)


def _d16(_lib, one, **kw):
    base = dict(struct_size=C.sizeof(_lib.Depth16Block), dtype=_lib.DTYPE_F16, planes=C.addressof(one), plane_stride=0, scale=1.0, flags=0)
    base.update(kw)
    return _lib.Depth16Block(**base)


def _refused(_lib, a, d, *words, frames="table", P=1, rc_want=-1):
    table = (C.c_int64 * 3)()          # one zeroed la3d_frame row on the host, 8-byte aligned: a refused call never reads it
    fr = C.addressof(table) if frames == "table" else frames
    rc = getattr(_lib.lib, NAME)(C.byref(a) if a is not None else None, C.byref(d) if d is not None else None, fr, P)
    err = _lib.lib.la3d_last_error()
    assert rc == rc_want, (rc, err)
    assert NAME.encode() in err, err
    for w in words:
        assert w in err, err


def test_c_entry_refuses_before_any_launch():
    from labelany3d_amd import _lib

    one = (C.c_double * 64)()
    p = C.addressof(one)
    assert p % 8 == 0
    U16 = _lib.DTYPE_U16
    UNSUP = _lib.ERR_UNSUPPORTED
    # a bad block or la3d_depth16: struct_size, dtype, planes, scale, flags
    _refused(_lib, None, _d16(_lib, one), b"struct_size")
    _refused(_lib, _block(_lib, one, struct_size=8), _d16(_lib, one), b"struct_size")
    _refused(_lib, _block(_lib, one), None, b"NULL")
    _refused(_lib, _block(_lib, one), _d16(_lib, one, struct_size=24), b"struct_size")
    _refused(_lib, _block(_lib, one), _d16(_lib, one, struct_size=0), b"struct_size")
    for dtype in (0, 2, 4, -1):
        _refused(_lib, _block(_lib, one), _d16(_lib, one, dtype=dtype), b"dtype")
    _refused(_lib, _block(_lib, one), _d16(_lib, one, planes=None), b"planes")
    _refused(_lib, _block(_lib, one), _d16(_lib, one, planes=p + 1), b"planes")
    for scale in (0.0, -0.001, float("inf"), float("nan")):
        _refused(_lib, _block(_lib, one), _d16(_lib, one, dtype=U16, scale=scale), b"scale")
    _refused(_lib, _block(_lib, one), _d16(_lib, one, flags=1), b"flags")
    for flags in (2, 3, -1, 256):
        _refused(_lib, _block(_lib, one), _d16(_lib, one, dtype=U16, scale=0.001, flags=flags), b"flags")
    # the planes come in the la3d_depth16 block, the frame table says where they lie
    _refused(_lib, _block(_lib, one, depth=p), _d16(_lib, one), b"args->depth")
    _refused(_lib, _block(_lib, one, depth_plane_stride=256), _d16(_lib, one), b"depth_plane_stride")
    _refused(_lib, _block(_lib, one, frame_width=16), _d16(_lib, one), b"frame_width")
    for stride in (256, 1, -1):
        _refused(_lib, _block(_lib, one), _d16(_lib, one, plane_stride=stride), b"plane_stride")
    # a misaligned base: 2- and 4-byte alignment is what the uniform entry takes, the ragged buffer needs 8
    for off in (2, 4, 6):
        _refused(_lib, _block(_lib, one), _d16(_lib, one, planes=p + off), b"8-byte aligned")
    # u8 and bit-plane masks, the hull method
    _refused(_lib, _block(_lib, one, mask=p), _d16(_lib, one), b"u8 mask planes", rc_want=UNSUP)
    _refused(_lib, _block(_lib, one, rle_counts=None, rle_offsets=None), _d16(_lib, one), b"rle_counts / poly_xy")   # what a bit-plane call hands over
    _refused(_lib, _block(_lib, one, poly_xy=p, ring_offsets=p, inst_rings=p), _d16(_lib, one), b"rle_counts / poly_xy")   # two sources
    _refused(_lib, _block(_lib, one, rle_counts=None, rle_offsets=None, poly_xy=p), _d16(_lib, one), b"ring_offsets")
    _refused(_lib, _block(_lib, one, method=_lib.METHOD_CONVEX_HULL), _d16(_lib, one), b"CONVEX_HULL", rc_want=UNSUP)
    _refused(_lib, _block(_lib, one, method=2), _d16(_lib, one), b"method")
    # the frame table and the image index
    _refused(_lib, _block(_lib, one, image_index=None), _d16(_lib, one), b"image_index")
    _refused(_lib, _block(_lib, one), _d16(_lib, one), b"frames", frames=None)
    _refused(_lib, _block(_lib, one), _d16(_lib, one), b"frames", frames=p + 4)
    _refused(_lib, _block(_lib, one), _d16(_lib, one), b"frames", P=0)
    _refused(_lib, _block(_lib, one), _d16(_lib, one), b"frames", P=-1)
    # what the block entries refuse stays refused
    _refused(_lib, _block(_lib, one, opt_engine=9), _d16(_lib, one), b"opt_engine")
    _refused(_lib, _block(_lib, one, workspace=None), _d16(_lib, one), b"workspace")
    # bounds beyond the tiled form: the bit image of 1024 x 1056 does not fit the LDS; H above 2040, W above 8160, in either mode
    _refused(_lib, _block(_lib, one, H=1024, W=1056), _d16(_lib, one), b"1048576", rc_want=UNSUP)
    _refused(_lib, _block(_lib, one, H=2048, W=64), _d16(_lib, one), b"tiled form", rc_want=UNSUP)
    _refused(_lib, _block(_lib, one, H=16, W=8192), _d16(_lib, one, dtype=U16, scale=0.001), b"tiled form", rc_want=UNSUP)
    _refused(_lib, _block(_lib, one, H=2048, W=64, sample_idx=p), _d16(_lib, one), b"subsample", b"tiled form", rc_want=UNSUP)
    # B = 0 returns 0 without a device
    for d in (_d16(_lib, one), _d16(_lib, one, dtype=U16, scale=0.001, flags=1)):
        a = _block(_lib, one, B=0, workspace=None, image_index=None)
        assert getattr(_lib.lib, NAME)(C.byref(a), C.byref(d), None, 0) == 0


MAPS = [(61, 75), (8, 32), (100, 214), (5, 7), (96, 224)]


def _maps(dtype, seed=3):
    """maps of the stored dtype holding every kind of word: NaN payloads, infinities, -0, subnormals (float16); 0 and 65535 (uint16)"""
    rs = np.random.RandomState(seed)
    out = []
    for h, w in MAPS:
        words = rs.randint(0, 65536, (h, w)).astype(np.uint16)
        words[0, 0], words[-1, -1], words[h // 2, w // 2] = 65535, 0, 0x7E01 if dtype == "f16" else 65535   # (0x7E01: a NaN with a payload)
        words[0, -1] = 0x8000 if dtype == "f16" else 1                                                    # -0
        out.append(words.view(np.float16) if dtype == "f16" else words)
    return out


@pytest.mark.parametrize("dtype", ["f16", "u16"])
def test_pack_frames_16bit_layout_on_the_host(dtype):
    import torch

    import labelany3d_amd as la
    from labelany3d_amd.masks import frame_table

    maps = _maps(dtype)
    tdt = torch.float16 if dtype == "f16" else torch.uint16
    for src in (maps, [torch.from_numpy(m.view(np.int16)).view(tdt) for m in maps]):
        pf = la.pack_frames(src, device="cpu", dtype=dtype, scale=0.00025, zero_is_hole=False)
        assert isinstance(pf, la.PackedFrames16) and pf.data.dtype == tdt and pf.data.dim() == 1 and not pf.data.is_cuda
        want = frame_table(MAPS)
        np.testing.assert_array_equal(pf.table_host, want)
        assert (pf.table_host["depth_offset"] % 4 == 0).all()
        np.testing.assert_array_equal(pf.table.numpy(), np.ascontiguousarray(want).view(np.int32).reshape(len(MAPS), 6))
        assert (pf.H, pf.W, pf.sizes) == (100, 224, MAPS)
        assert (pf.scale, pf.zero_is_hole) == ((0.00025, False) if dtype == "u16" else (1.0, False))
        words = pf.data.view(torch.int16).numpy().view(np.uint16)
        total = int(want["depth_offset"][-1]) + int(want["H"][-1]) * int(want["W"][-1])
        assert words.size == total                                    # an exactly sized buffer
        seen = np.zeros(total, bool)
        for m, r in zip(maps, want):
            o, h, wp, w = int(r["depth_offset"]), int(r["H"]), int(r["W"]), int(r["frame_width"])
            plane = words[o:o + h * wp].reshape(h, wp)
            np.testing.assert_array_equal(plane[:, :w], m.view(np.uint16))   # bit-identical: NaN payloads, -0, 65535
            assert (plane[:, w:] == 0).all()                                 # zero words in the padding columns
            seen[o:o + h * wp] = True
        assert seen.all()
    # a pinned-style staging tensor of the 16-bit dtype is used when it is large enough
    stage = torch.full((total + 64,), 7, dtype=torch.int16).view(tdt)
    pf2 = la.pack_frames(maps, device="cpu", dtype=dtype, pinned=stage)
    assert pf2.data.data_ptr() == stage.data_ptr()
    np.testing.assert_array_equal(pf2.data.view(torch.int16).numpy(), pf.data.view(torch.int16).numpy())
    # dtype=None is the float32 function
    pf32 = la.pack_frames([m.astype(np.float32) for m in _maps("u16")], device="cpu")
    assert isinstance(pf32, la.PackedFrames) and pf32.depth.dtype == torch.float32
    np.testing.assert_array_equal(pf32.table_host, want)


def test_pack_frames_16bit_argument_errors():
    import torch

    import labelany3d_amd as la

    good = np.zeros((8, 32), np.uint16)
    for dtype, bad in (("u16", np.zeros((8, 32), np.float32)), ("u16", np.zeros((8, 32), np.float16)), ("u16", np.zeros((8, 32), np.int16)),
                       ("f16", np.zeros((8, 32), np.uint16)), ("f16", np.zeros((8, 32), np.float64)),
                       ("f16", torch.zeros((8, 32), dtype=torch.bfloat16)), ("u16", torch.zeros((8, 32), dtype=torch.float16))):
        with pytest.raises(ValueError, match="depth map 1"):
            la.pack_frames([good if dtype == "u16" else good.view(np.float16), bad], device="cpu", dtype=dtype)
    with pytest.raises(ValueError, match="dtype"):
        la.pack_frames([good], device="cpu", dtype="bf16")
    for scale in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="scale"):
            la.pack_frames([good], device="cpu", dtype="u16", scale=scale)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        la.pack_frames([good[None]], device="cpu", dtype="u16")


def test_fit_instances_frames_argument_errors_before_any_device_work():
    import torch

    import labelany3d_amd as la

    K = np.eye(3)
    u = la.pack_frames([np.ones((8, 32), np.uint16)], device="cpu", dtype="u16")
    h = la.pack_frames([np.ones((8, 32), np.float16)], device="cpu", dtype="f16")
    ii = np.zeros(0, np.int32)
    for pf in (u, h):
        with pytest.raises(ValueError, match="convex_hull"):                      # the frames entry's refusals ...
            la.fit_instances_frames(pf, K, rles=[], image_index=ii, method="convex_hull")
        with pytest.raises(ValueError, match="exactly one of rles / polys"):
            la.fit_instances_frames(pf, K, image_index=ii)
        with pytest.raises(ValueError, match="exactly one of rles / polys"):
            la.fit_instances_frames(pf, K, rles=[], polys=(np.zeros(2, np.int32), np.zeros(1, np.int64), np.zeros(1, np.int64), 8, 32), image_index=ii)
        with pytest.raises(ValueError, match="image_index is required"):
            la.fit_instances_frames(pf, K, rles=[])
        with pytest.raises(ValueError, match="live on the GPU"):
            la.fit_instances_frames(pf, K, rles=[], image_index=ii)
    for scale in (0.0, -0.001, float("nan"), float("inf"), 1e-60):                # ... and those of a Depth16
        with pytest.raises(ValueError, match="scale"):
            la.fit_instances_frames(u._replace(scale=scale), K, rles=[], image_index=ii)
    for bad in (torch.zeros(256, dtype=torch.float32), torch.zeros(256, dtype=torch.int16), torch.zeros(256, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="float16 or torch.uint16"):
            la.fit_instances_frames(u._replace(data=bad), K, rles=[], image_index=ii)
    with pytest.raises(ValueError, match="flat tensor"):
        la.fit_instances_frames(u._replace(data=u.data.view(8, 32)), K, rles=[], image_index=ii)
    with pytest.raises(ValueError, match="float32 depth planes only"):            # a bare Depth16 is not a frames argument
        la.fit_instances_frames(la.Depth16(torch.zeros((1, 8, 32), dtype=torch.float16)), K, rles=[])
    with pytest.raises(ValueError, match="PackedFrames"):
        la.fit_instances_frames(np.zeros((8, 32), np.float16), K, rles=[], image_index=ii)


def test_scene_pipeline_depth_dtype_errors():
    import labelany3d_amd as la
    from labelany3d_amd import fit_scenes as FS

    for bad in ("bf16", "f32", "float16", 16):
        with pytest.raises(ValueError, match="depth_dtype"):                      # refused before the device is looked for
            FS.ScenePipeline(depth_dtype=bad)
    for scale in (0.0, float("nan")):
        with pytest.raises(ValueError, match="depth_scale"):
            FS.ScenePipeline(depth_dtype="u16", depth_scale=scale)
    k = np.zeros(9)
    K = np.eye(3).tolist()
    for want, depth in ((np.uint16, np.ones((8, 32), np.float32)), (np.uint16, np.ones((8, 32), np.float16)), (np.float16, np.ones((8, 32), np.uint16)),
                        (np.float16, np.ones((8, 32), np.float32)), (np.uint16, np.ones((8, 32), np.int16)), (np.float16, [[1.0] * 32] * 8)):
        with pytest.raises(ValueError, match="scene-7.*depth_dtype"):
            FS._load_scene(dict(name="scene-7", depth=depth, K=K), np.zeros((8, 32), want), k, np.dtype(want))
    for want in (np.uint16, np.float16):                                         # the right dtype goes in bit for bit, rows of a padded plane too
        src = (np.arange(256, dtype=np.uint16).reshape(8, 32) * 257).view(want)
        for out in (np.zeros((8, 32), want), np.zeros((8, 64), want)[:, :32]):
            FS._load_scene(dict(name="s", depth=src, K=K), out, k, np.dtype(want))
            np.testing.assert_array_equal(out.view(np.uint16), src.view(np.uint16))
    np.testing.assert_array_equal(k, np.eye(3).reshape(9))
    import torch
    with pytest.raises(ValueError, match="float32 depth planes only"):            # a Depth16 OBJECT as a scene's depth stays refused
        list(FS.ScenePipeline._batches(type("S", (), dict(mixed_frames=True, batch_images=4))(),
                                       [dict(depth=la.Depth16(torch.zeros((8, 32), dtype=torch.float16)), height=8, width=32)]))
    ap = FS.build_parser()
    a = ap.parse_args(["--scenes", "x"])
    assert (a.depth_dtype, a.depth_scale, a.depth_keep_zero) == ("f32", 0.001, False)
    a = ap.parse_args(["--scenes", "x", "--depth-dtype", "u16", "--depth-scale", "0.00025", "--depth-keep-zero"])
    assert (a.depth_dtype, a.depth_scale, a.depth_keep_zero) == ("u16", 0.00025, True)


@pytest.mark.parametrize("dtype,scale", [("u16", 0.001), ("u16", 0.00025), ("f16", 1.0)])
def test_synthetic_scenes_in_16_bit(tmp_path, dtype, scale):
    from labelany3d_amd.fit_scenes import quantise_depth, synthetic_scenes

    ref, _ = synthetic_scenes(3, seed=9, H=61, W=75)
    got, data = synthetic_scenes(3, seed=9, H=61, W=75, root=str(tmp_path), depth_dtype=dtype, depth_scale=scale)
    ndt = np.uint16 if dtype == "u16" else np.float16
    for r, g in zip(ref, got):
        assert g["depth"].dtype == ndt and g["annotations"] == r["annotations"] and g["K"] == r["K"]
        stored = DC.quantise(r["depth"], dtype, scale)
        np.testing.assert_array_equal(g["depth"].view(np.uint16), stored.view(np.uint16))
        on_disk = np.load(os.path.join(str(tmp_path), g["name"], "depth_map.npy"))
        assert on_disk.dtype == ndt
        np.testing.assert_array_equal(DC.upconvert(on_disk, scale, True), DC.upconvert(stored, scale, True))
        assert np.isfinite(DC.upconvert(on_disk, scale, True)).all()
    d = np.array([np.nan, np.inf, -1.0, 0.0, 0.0004, 0.0015, 0.0025, 70.0, 6e-8, 65520.0], np.float32)    # the edge values of the rule
    for dt in ("u16", "f16"):
        np.testing.assert_array_equal(quantise_depth(d, dt, 0.001).view(np.uint16), DC.quantise(d, dt, 0.001).view(np.uint16))
    with pytest.raises(ValueError, match="depth_dtype"):
        synthetic_scenes(1, depth_dtype="bf16")
