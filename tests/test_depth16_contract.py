"""CPU-only contract of the 16-bit depth source (include/la3d.h "16-bit depth planes"): the exports exist on every layer, the layout
of ``la3d_depth16``, every call-level refusal of ``la3d_fit_instances_depth16`` before any launch (host dummies stand in for the
device pointers: a refused call never touches them), the Python argument errors before any device work, and the well-posedness of
the GPU cases: the oracle alone, on the up-converted planes, passes every comparison tests/test_gpu_depth16.py makes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import depth16_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("la3d_fit_instances_depth16", "la3d_pack_depth16", "la3d_unpack_depth16")


def test_new_symbols_on_every_layer():
    from labelany3d_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    declared = set(re.findall(r"\b(la3d_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and hasattr(_lib.lib, name) and name in _lib.EXPORTS, name
    for macro in ("LA3D_DTYPE_U16 3", "LA3D_DEPTH_ZERO_IS_HOLE 1", "LA3D_DTYPE_F16 1"):
        assert re.search(r"#define\s+" + macro.replace(" ", r"\s+") + r"\b", hdr), macro
    assert (_lib.DTYPE_F16, _lib.DTYPE_U16, _lib.DEPTH_ZERO_IS_HOLE) == (1, 3, 1)
    assert _lib.lib.la3d_version() == 2 and C.sizeof(_lib.FitArgs) == 232       # new exports only: the block does not grow
    import labelany3d_amd as la
    for fn in ("Depth16", "pack_depth16", "unpack_depth16"):
        assert callable(getattr(la, fn)) and fn in la.__all__
    assert la.Depth16._fields == ("data", "scale", "zero_is_hole", "frame_width")
    assert la.Depth16._field_defaults == dict(scale=1.0, zero_is_hole=True, frame_width=0)


def test_depth16_block_layout():
    from labelany3d_amd import _lib

    D = _lib.Depth16Block
    assert C.sizeof(D) == 32
    offs = {n: getattr(D, n).offset for n, _ in D._fields_}
    assert offs == dict(struct_size=0, dtype=4, planes=8, plane_stride=16, scale=24, flags=28)
    assert [n for n, _ in D._fields_] == ["struct_size", "dtype", "planes", "plane_stride", "scale", "flags"]


def _block(_lib, one, **kw):
    p = C.addressof(one)
    base = dict(struct_size=C.sizeof(_lib.FitArgs), B=1, H=8, W=32, mask=p, K=p, out=p, status=p, workspace=p)
    base.update(kw)
    return _lib.FitArgs(**base)


def _d16(_lib, one, **kw):
    base = dict(struct_size=C.sizeof(_lib.Depth16Block), dtype=_lib.DTYPE_F16, planes=C.addressof(one), plane_stride=0, scale=1.0, flags=0)
    base.update(kw)
    return _lib.Depth16Block(**base)


def _refused(_lib, a, d, *words, bits=None, stride=0, flags=0, rc_want=-1):
    rc = _lib.lib.la3d_fit_instances_depth16(C.byref(a) if a is not None else None, C.byref(d) if d is not None else None, bits, stride, flags)
    err = _lib.lib.la3d_last_error()
    assert rc == rc_want, (rc, err)
    assert b"la3d_fit_instances_depth16" in err, err
    for w in words:
        assert w in err, err


def test_c_entry_refuses_before_any_launch():
    from labelany3d_amd import _lib

    one = (C.c_double * 64)()
    p = C.addressof(one)
    U16 = _lib.DTYPE_U16
    _refused(_lib, None, _d16(_lib, one), b"struct_size")                                    # NULL block
    _refused(_lib, _block(_lib, one, struct_size=8), _d16(_lib, one), b"struct_size")
    _refused(_lib, _block(_lib, one), None, b"NULL")                                         # NULL la3d_depth16
    _refused(_lib, _block(_lib, one), _d16(_lib, one, planes=None), b"planes")               # NULL planes
    _refused(_lib, _block(_lib, one), _d16(_lib, one, planes=p + 1), b"planes")              # not 2-byte aligned
    _refused(_lib, _block(_lib, one), _d16(_lib, one, struct_size=24), b"struct_size")
    _refused(_lib, _block(_lib, one), _d16(_lib, one, struct_size=0), b"struct_size")
    for dtype in (0, 2, 4, -1):                                                              # F32, BF16, unknown
        _refused(_lib, _block(_lib, one), _d16(_lib, one, dtype=dtype), b"dtype")
    _refused(_lib, _block(_lib, one, depth=p), _d16(_lib, one), b"args->depth")              # depth given twice
    _refused(_lib, _block(_lib, one, depth_plane_stride=256), _d16(_lib, one), b"depth_plane_stride")
    for scale in (0.0, -0.001, float("inf"), float("nan")):
        _refused(_lib, _block(_lib, one), _d16(_lib, one, dtype=U16, scale=scale), b"scale")
    _refused(_lib, _block(_lib, one), _d16(_lib, one, flags=1), b"flags")                    # a flag on float16 planes
    for flags in (2, 3, -1, 256):
        _refused(_lib, _block(_lib, one), _d16(_lib, one, dtype=U16, scale=0.001, flags=flags), b"flags")
    _refused(_lib, _block(_lib, one), _d16(_lib, one, plane_stride=255), b"plane_stride")    # < H*W
    _refused(_lib, _block(_lib, one), _d16(_lib, one, plane_stride=-1), b"plane_stride")
    _refused(_lib, _block(_lib, one, mask=None), _d16(_lib, one), b"mask source")            # no mask source
    for second in ("rle_counts", "poly_xy"):                                                 # two mask sources
        _refused(_lib, _block(_lib, one, **{second: p, "rle_offsets": p, "ring_offsets": p, "inst_rings": p}), _d16(_lib, one), b"mask source")
    _refused(_lib, _block(_lib, one), _d16(_lib, one), b"mask source", bits=p, stride=8)     # u8 planes and bit planes
    _refused(_lib, _block(_lib, one, mask=None, rle_counts=p, rle_offsets=p), _d16(_lib, one), b"mask source", bits=p, stride=8)
    # the bit-plane arguments follow la3d_fit_instances_bits
    _refused(_lib, _block(_lib, one, mask=None), _d16(_lib, one), b"bits_plane_stride", bits=p, stride=7)
    _refused(_lib, _block(_lib, one, mask=None), _d16(_lib, one), b"bits_flags", bits=p, stride=8, flags=2)
    _refused(_lib, _block(_lib, one, mask=None), _d16(_lib, one), b"mask_bits", bits=p + 2, stride=8)
    # what the block entries refuse stays refused
    _refused(_lib, _block(_lib, one, method=2), _d16(_lib, one), b"method")
    _refused(_lib, _block(_lib, one, opt_engine=9), _d16(_lib, one), b"opt_engine")
    _refused(_lib, _block(_lib, one, proj=p), _d16(_lib, one), b"image_width")
    _refused(_lib, _block(_lib, one, workspace=None), _d16(_lib, one), b"workspace")
    _refused(_lib, _block(_lib, one, frame_width=16), _d16(_lib, one), b"frame_width")       # padded rows: not with u8 planes
    _refused(_lib, _block(_lib, one, mask=None, H=1024, W=1056), _d16(_lib, one), b"1048576", bits=p, stride=1024 * 1056 // 32, rc_want=-2)
    # a well-formed call of no instances succeeds without a device
    a = _block(_lib, one, B=0, workspace=None)
    assert _lib.lib.la3d_fit_instances_depth16(C.byref(a), C.byref(_d16(_lib, one)), None, 0, 0) == 0
    assert _lib.lib.la3d_fit_instances_depth16(C.byref(a), C.byref(_d16(_lib, one, dtype=U16, scale=0.001, flags=1)), None, 0, 0) == 0


def test_packer_argument_errors_without_a_device():
    from labelany3d_amd import _lib

    L = _lib.lib
    one = (C.c_double * 64)()
    p = C.addressof(one)

    def refused(rc, name, *words):
        err = L.la3d_last_error()
        assert rc == -1 and name in err, (rc, err)
        for w in words:
            assert w in err, err

    refused(L.la3d_pack_depth16(p, 256, 1, 8, 32, 32, 0, 0.001, p, 256, None), b"la3d_pack_depth16", b"dtype")
    refused(L.la3d_pack_depth16(p, 256, 1, 8, 32, 32, 2, 0.001, p, 256, None), b"la3d_pack_depth16", b"dtype")
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        refused(L.la3d_pack_depth16(p, 256, 1, 8, 32, 32, 3, scale, p, 256, None), b"la3d_pack_depth16", b"scale")
    refused(L.la3d_pack_depth16(p, 256, 1, 8, 32, 31, 1, 1.0, p, 256, None), b"la3d_pack_depth16", b"W_out")
    refused(L.la3d_pack_depth16(None, 256, 1, 8, 32, 32, 1, 1.0, p, 256, None), b"la3d_pack_depth16")
    refused(L.la3d_pack_depth16(p, 256, 1, 8, 32, 32, 1, 1.0, p + 1, 256, None), b"la3d_pack_depth16", b"aligned")
    refused(L.la3d_pack_depth16(p, 256, 2, 8, 32, 64, 1, 1.0, p, 511, None), b"la3d_pack_depth16", b"stride")
    assert L.la3d_pack_depth16(None, 0, 0, 8, 32, 32, 1, 1.0, None, 0, None) == 0
    refused(L.la3d_unpack_depth16(None, 1, 8, 32, 32, p, None), b"la3d_unpack_depth16", b"struct_size")
    refused(L.la3d_unpack_depth16(C.byref(_d16(_lib, one, dtype=0)), 1, 8, 32, 32, p, None), b"la3d_unpack_depth16", b"dtype")
    refused(L.la3d_unpack_depth16(C.byref(_d16(_lib, one, flags=1)), 1, 8, 32, 32, p, None), b"la3d_unpack_depth16", b"flags")
    refused(L.la3d_unpack_depth16(C.byref(_d16(_lib, one, dtype=3, scale=0.0)), 1, 8, 32, 32, p, None), b"la3d_unpack_depth16", b"scale")
    refused(L.la3d_unpack_depth16(C.byref(_d16(_lib, one)), 1, 8, 32, 33, p, None), b"la3d_unpack_depth16", b"W_in")
    refused(L.la3d_unpack_depth16(C.byref(_d16(_lib, one, plane_stride=255)), 2, 8, 32, 32, p, None), b"la3d_unpack_depth16", b"plane_stride")
    assert L.la3d_unpack_depth16(C.byref(_d16(_lib, one)), 0, 8, 32, 32, None, None) == 0


def test_python_argument_errors_before_any_device_work():
    import torch

    import labelany3d_amd as la
    from labelany3d_amd import shard

    K = np.eye(3)
    masks = np.zeros((2, 8, 32), bool)
    h = torch.zeros((2, 8, 32), dtype=torch.float16)
    u = torch.zeros((2, 8, 32), dtype=torch.uint16)
    for bad in (torch.zeros((2, 8, 32), dtype=torch.float32), torch.zeros((2, 8, 32), dtype=torch.int16),
                torch.zeros((2, 8, 32), dtype=torch.bfloat16), np.zeros((2, 8, 32), np.float16)):
        with pytest.raises(ValueError, match="float16 or torch.uint16"):
            la.fit_instances(la.Depth16(bad), masks, K)
        with pytest.raises(ValueError, match="float16 or torch.uint16"):
            la.fit_instances_ex(la.Depth16(bad), K, masks=masks)
        with pytest.raises(ValueError, match="float16 or torch.uint16"):
            la.fit_instances_bits(la.Depth16(bad), None, K)
    for scale in (0.0, -0.001, float("nan"), float("inf"), 1e-60):   # (1e-60 is 0 as float32)
        with pytest.raises(ValueError, match="scale"):
            la.fit_instances(la.Depth16(u, scale), masks, K)
        with pytest.raises(ValueError, match="scale"):
            la.fit_instances_rle(la.Depth16(u, scale), [], K)
        with pytest.raises(ValueError, match="scale"):
            la.pack_depth16(np.zeros((8, 32), np.float32), "u16", scale)
    with pytest.raises(ValueError, match="dtype"):
        la.pack_depth16(np.zeros((8, 32), np.float32), "bf16")
    for d in (h, u, h[0]):                                            # shape mismatch with the masks
        with pytest.raises(ValueError, match="do not match"):
            la.fit_instances(la.Depth16(d), np.zeros((2, 8, 64), bool), K)
    with pytest.raises(ValueError, match=r"\(P,H,W\) or \(H,W\)"):
        la.fit_instances(la.Depth16(h[None]), masks, K)
    with pytest.raises(ValueError, match="frame_width"):
        la.fit_instances(la.Depth16(h, frame_width=33), masks, K)
    # the entries without a 16-bit form name the limit
    for call in (lambda: la.fit_instances_frames(la.Depth16(h), K, rles=[]),
                 lambda: la.fit_annotations([], (32, 8), la.Depth16(h), K),
                 lambda: la.fit_annotations_all([], (32, 8), la.Depth16(u, 0.001), K),
                 lambda: shard.fit_instances_sharded(la.Depth16(h), masks, K, np.zeros(2, np.int32))):
        with pytest.raises(ValueError, match="float32 depth planes only"):
            call()
    with pytest.raises(ValueError, match="float32 depth planes only"):
        from labelany3d_amd.fit_scenes import ScenePipeline
        list(ScenePipeline._batches(type("S", (), dict(mixed_frames=False, batch_images=4))(), [dict(depth=la.Depth16(h), height=8, width=32)]))
    # a plain 16-bit array is NOT a Depth16: it keeps today's route (up-converted to float32), so it needs no new check here


def test_numpy_value_rules():
    """the definitions the tests use, on the edge values: what ``quantise`` / ``upconvert`` say must be what the header says"""
    d = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 0.0004, 0.0005, 0.0015, 0.0025, 65.535, 65.5354, 70.0, 6e-8, 65504.0, 65520.0], np.float32)
    u = DC.quantise(d, "u16", 0.001)
    np.testing.assert_array_equal(u, [0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 65535, 65535, 65535, 0, 65535, 65535])   # (0.0005f / 0.001f is just below 0.5; 0.0015 and 0.0025 both go to 2)
    f = DC.quantise(d, "f16")
    assert f.dtype == np.float16 and np.isnan(f[0]) and np.isinf(f[1]) and f[13] == np.float16(6e-8) and f[13] > 0 and f[14] == 65504 and np.isinf(f[15])
    up = DC.upconvert(np.array([0, 1, 3, 65535], np.uint16), 0.001, True)
    assert np.isnan(up[0]) and up[1] == np.float32(0.001) and up[2] == np.float32(3) * np.float32(0.001) and up.dtype == np.float32
    x = np.arange(65536, dtype=np.uint16)                               # one float32 rounding of x * float32(scale): for thousands of words
    assert (DC.upconvert(x, 0.001, False) != (x.astype(np.float64) * 0.001).astype(np.float32)).sum() > 1000   # not the rounded exact product
    assert DC.upconvert(np.array([0], np.uint16), 0.001, False)[0] == 0.0
    hf = np.array([6e-8, -0.0, np.inf, np.nan, 65504], np.float16)
    uf = DC.upconvert(hf)
    assert uf[0] == np.float32(2.0 ** -24) and np.signbit(uf[1]) and np.isinf(uf[2]) and np.isnan(uf[3]) and uf[4] == 65504


CASES = DC.fixed_cases()


@pytest.mark.parametrize("variant", DC.VARIANTS, ids=DC.VARIANT_IDS)
def test_gpu_cases_are_well_posed(variant):
    """The oracle on the up-converted planes of every fixed case: status 0 everywhere except the instances built to be rejected, and
    no fitted instance with an eigen-gap of exactly 0 (the suite's documented don't-care) - so the reference alone passes every
    comparison the GPU test makes."""
    seen = set()
    for case in CASES:
        assert case["name"] not in seen
        seen.add(case["name"])
        stored, up, want, sidx = DC.materialise(case, variant)
        assert stored.dtype == (np.float16 if variant[0] == "f16" else np.uint16) and up.dtype == np.float32
        st, gap = DC.oracle_gaps(up, case["masks"], case["K"], case["ground"], sidx, case["ii"], case["method"])
        np.testing.assert_array_equal(st, want, err_msg=case["name"])
        assert (want == 0).sum() >= len(want) // 2, case["name"]
        fitted = st == 0
        assert np.isfinite(gap[fitted]).all() and (gap[fitted] > 0).all(), (case["name"], gap)
        rec, st2, _, _ = DC.O.fit_instances(up, case["masks"], case["K"], ground=case["ground"], sample_idx=sidx, depth_index=case["ii"],
                                            method=case["method"])
        np.testing.assert_array_equal(st2, want, err_msg=case["name"])
        assert np.isfinite(rec[fitted]).all(), f"{case['name']}: a fitted record of the oracle is not finite (float16 overflow of a corner)"
        if case["sample"]:
            counts = case["masks"].reshape(len(want), -1).sum(1)
            assert (counts > DC.NSAMPLE).any() and ((counts > 0) & (counts <= DC.NSAMPLE)).any(), case["name"]
        if case["name"].startswith("pivot"):
            _, _, _, _, kappa = DC.O.fit_instances(up, case["masks"], case["K"], return_kappa=True)
            assert (kappa > 2.0 ** 17).all(), (case["name"], kappa)
