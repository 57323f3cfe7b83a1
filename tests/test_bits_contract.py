"""CPU-only contract of the bit-plane mask source (include/la3d.h "masks as bit planes"): the new exports exist on every layer,
la3d_mask_bits_words is ceil(H*W/32), and every argument error of the new entries is reported before any device work (host
dummies stand in for the device pointers: a call that is refused never touches them)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("la3d_fit_instances_bits", "la3d_mask_bits_words", "la3d_pack_mask_bits", "la3d_pack_logits_bits", "la3d_unpack_mask_bits",
       "la3d_mask_stats_bits")
MSG = r"Unknown method: obb\. Use 'pca' or 'convex_hull'"


def test_new_symbols_on_every_layer():
    from labelany3d_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    declared = set(re.findall(r"\b(la3d_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in la3d.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported by libla3d.so"
        assert name in _lib.EXPORTS
    assert _lib.lib.la3d_version() == 2                     # new exports only: the ABI number and the block stay
    assert _lib.FitArgs._fields_[-1][0] == "method"
    for macro in ("LA3D_BITS_HEIGHT_ROWS 0", "LA3D_BITS_HEIGHT_SPAN 1", "LA3D_DTYPE_F32 0", "LA3D_DTYPE_F16 1", "LA3D_DTYPE_BF16 2"):
        assert re.search(r"#define\s+" + macro.replace(" ", r"\s+") + r"\b", hdr), macro
    import labelany3d_amd as la
    for fn in ("fit_instances_bits", "pack_mask_bits", "pack_logits_bits", "unpack_mask_bits", "mask_stats_bits"):
        assert callable(getattr(la, fn)) and fn in la.__all__
    assert callable(la.InstanceFitter.run_bits)


@pytest.mark.parametrize("H,W", [(480, 640), (8, 32), (37, 53), (100, 214), (1, 1), (1, 33), (517, 672), (3, 21), (1024, 1024)])
def test_mask_bits_words(H, W):
    from labelany3d_amd import _lib

    assert _lib.lib.la3d_mask_bits_words(H, W) == -(-(H * W) // 32)
    packed = np.packbits(np.ones((1, H * W), bool), axis=1, bitorder="little")
    assert _lib.lib.la3d_mask_bits_words(H, W) == -(-packed.shape[1] // 4)     # the uint32 view of np.packbits, rounded up


def test_mask_bits_words_of_no_frame_is_zero():
    from labelany3d_amd import _lib

    assert _lib.lib.la3d_mask_bits_words(0, 640) == 0 and _lib.lib.la3d_mask_bits_words(480, -1) == 0


def _block(_lib, one, **kw):
    p = C.addressof(one)
    base = dict(struct_size=C.sizeof(_lib.FitArgs), B=1, H=8, W=32, depth=p, K=p, out=p, status=p, workspace=p)
    base.update(kw)
    return _lib.FitArgs(**base)


def _refused(_lib, rc_want, a, bits, stride, flags, *words):
    rc = _lib.lib.la3d_fit_instances_bits(C.byref(a) if a is not None else None, bits, stride, flags)
    err = _lib.lib.la3d_last_error()
    assert rc == rc_want, (rc, err)
    assert b"la3d_fit_instances_bits" in err, err
    for w in words:
        assert w in err, err


def test_fit_bits_argument_errors_without_a_device():
    from labelany3d_amd import _lib

    one = (C.c_double * 64)()
    p = C.addressof(one)
    nw = 8 * 32 // 32
    _refused(_lib, -1, None, p, nw, 0, b"struct_size")
    _refused(_lib, -1, _block(_lib, one, struct_size=8), p, nw, 0, b"struct_size")
    _refused(_lib, -1, _block(_lib, one), None, nw, 0, b"mask_bits")                      # NULL planes with B > 0
    _refused(_lib, -1, _block(_lib, one), p + 2, nw, 0, b"mask_bits")                     # not 4-byte aligned
    for second in ("mask", "rle_counts", "poly_xy"):                                       # a second mask source in the block
        _refused(_lib, -1, _block(_lib, one, **{second: p}), p, nw, 0, b"NULL")
    _refused(_lib, -1, _block(_lib, one), p, nw - 1, 0, b"bits_plane_stride")
    _refused(_lib, -1, _block(_lib, one, H=37, W=53), p, 37 * 53 // 32, 0, b"bits_plane_stride")   # needs ceil(1961 / 32) = 62
    for flags in (2, 4, -1, 3):
        _refused(_lib, -1, _block(_lib, one), p, nw, flags, b"flags")
    _refused(_lib, -1, _block(_lib, one, method=2), p, nw, 0, b"method")
    _refused(_lib, -1, _block(_lib, one, opt_engine=9), p, nw, 0, b"opt_engine")
    _refused(_lib, -1, _block(_lib, one, proj=p), p, nw, 0, b"image_width")
    _refused(_lib, -1, _block(_lib, one, depth=None), p, nw, 0)
    _refused(_lib, -1, _block(_lib, one, workspace=None), p, nw, 0, b"workspace")
    # frame_width follows the rule of run lengths / polygons: in (0, W], and W a multiple of 32 when it is smaller than W
    _refused(_lib, -1, _block(_lib, one, frame_width=33), p, nw, 0, b"frame_width")
    _refused(_lib, -1, _block(_lib, one, frame_width=-1), p, nw, 0, b"frame_width")
    _refused(_lib, -1, _block(_lib, one, H=8, W=40, frame_width=37), p, 10, 0, b"frame_width")
    # the fused filter is on with boundary >= 0 and max_edge > 0 only; boundary < 0 is simply "no filter" for a block entry
    # frames whose bit image does not fit LDS
    _refused(_lib, -2, _block(_lib, one, H=1024, W=1056), p, 1024 * 1056 // 32, 0, b"1048576")


def test_fit_bits_of_no_instances_succeeds_without_a_device():
    from labelany3d_amd import _lib

    one = (C.c_double * 64)()
    a = _block(_lib, one, B=0, workspace=None)
    assert _lib.lib.la3d_fit_instances_bits(C.byref(a), None, 0, 0) == 0
    assert _lib.lib.la3d_fit_instances_bits(C.byref(a), None, 0, 1) == 0
    assert _lib.lib.la3d_fit_instances_bits(C.byref(a), None, 0, 2) == -1               # (flags are checked whatever B is)


def test_packer_argument_errors_without_a_device():
    from labelany3d_amd import _lib

    L = _lib.lib
    one = (C.c_double * 64)()
    p = C.addressof(one)

    def refused(rc, want, name, *words):
        err = L.la3d_last_error()
        assert rc == want and name in err, (rc, err)
        for w in words:
            assert w in err, err

    refused(L.la3d_pack_mask_bits(p, 256, 1, 8, 32, 31, p, 8, None), -1, b"la3d_pack_mask_bits", b"W_out")
    refused(L.la3d_pack_mask_bits(None, 256, 1, 8, 32, 32, p, 8, None), -1, b"la3d_pack_mask_bits", b"NULL")
    refused(L.la3d_pack_mask_bits(p, 255, 2, 8, 32, 32, p, 8, None), -1, b"la3d_pack_mask_bits", b"stride")
    refused(L.la3d_pack_mask_bits(p, 256, 1, 8, 32, 32, p, 7, None), -1, b"la3d_pack_mask_bits", b"bits_plane_stride")
    refused(L.la3d_pack_mask_bits(p, 256, 1, 8, 32, 64, p, 15, None), -1, b"la3d_pack_mask_bits", b"bits_plane_stride")
    refused(L.la3d_pack_mask_bits(p, 256, 1, 8, 32, 32, p + 1, 8, None), -1, b"la3d_pack_mask_bits", b"aligned")
    refused(L.la3d_pack_mask_bits(p, 256, -1, 8, 32, 32, p, 8, None), -1, b"la3d_pack_mask_bits")
    assert L.la3d_pack_mask_bits(None, 0, 0, 8, 32, 32, None, 0, None) == 0
    refused(L.la3d_pack_logits_bits(p, 3, 256, 0.0, 1, 8, 32, 32, p, 8, None), -1, b"la3d_pack_logits_bits", b"dtype")
    refused(L.la3d_pack_logits_bits(p + 2, 0, 256, 0.0, 1, 8, 32, 32, p, 8, None), -1, b"la3d_pack_logits_bits", b"aligned")
    refused(L.la3d_pack_logits_bits(p, 1, 256, 0.0, 1, 8, 32, 32, p, 7, None), -1, b"la3d_pack_logits_bits", b"bits_plane_stride")
    assert L.la3d_pack_logits_bits(None, 2, 0, 0.5, 0, 8, 32, 32, None, 0, None) == 0
    refused(L.la3d_unpack_mask_bits(p, 8, 1, 8, 32, 33, p, None), -1, b"la3d_unpack_mask_bits")
    refused(L.la3d_unpack_mask_bits(p, 7, 1, 8, 32, 32, p, None), -1, b"la3d_unpack_mask_bits")
    assert L.la3d_unpack_mask_bits(None, 0, 0, 8, 32, 32, None, None) == 0
    refused(L.la3d_mask_stats_bits(p, 8, 1, 8, 32, 33, 10, p, None), -1, b"la3d_mask_stats_bits", b"frame_width")
    refused(L.la3d_mask_stats_bits(p, 8, 1, 8, 32, 0, -1, p, None), -1, b"la3d_mask_stats_bits")
    refused(L.la3d_mask_stats_bits(p, 7, 1, 8, 32, 0, 10, p, None), -1, b"la3d_mask_stats_bits")
    refused(L.la3d_mask_stats_bits(p, 40000, 1, 1024, 1056, 0, 10, p, None), -2, b"la3d_mask_stats_bits", b"1048576")
    assert L.la3d_mask_stats_bits(None, 0, 0, 8, 32, 0, 10, None, None) == 0


def test_unknown_method_and_height_rule_raise_before_any_device_work():
    import labelany3d_amd as la

    d, K = np.zeros((8, 32), np.float32), np.eye(3)
    with pytest.raises(ValueError, match=MSG):
        la.fit_instances_bits(d, None, K, method="obb")
    with pytest.raises(ValueError, match="height_rule"):
        la.fit_instances_bits(d, None, K, height_rule="tallest")
    with pytest.raises(ValueError, match="bits must be"):
        la.fit_instances_bits(d, None, K)
