"""CPU-only contract of the label-map mask source (include/la3d.h "masks as label maps"): the new export exists on every layer, the
ABI number and the argument block are the parent's, every ``ValueError`` of the Python layer is raised before any device work (NumPy
arguments on a machine without a GPU), and every argument error of the C entry is reported before any device work (host dummies
stand in for the device pointers: a call that is refused never touches them)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSG = r"Unknown method: obb\. Use 'pca' or 'convex_hull'"


def test_new_symbol_on_every_layer():
    from labelany3d_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    declared = set(re.findall(r"\b(la3d_[a-z0-9_]+)\s*\(", hdr))
    assert "la3d_pack_label_bits" in declared
    assert hasattr(_lib.lib, "la3d_pack_label_bits") and "la3d_pack_label_bits" in _lib.EXPORTS
    assert "masks as label maps" in hdr
    for macro, name, value in (("LA3D_LABEL_U8", "LABEL_U8", 0), ("LA3D_LABEL_U16", "LABEL_U16", 1), ("LA3D_LABEL_I32", "LABEL_I32", 2),
                               ("LA3D_LABEL_RGB8", "LABEL_RGB8", 3)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", hdr), macro
        assert getattr(_lib, name) == value
    # a new export only: the ABI number and the argument block stay
    assert _lib.lib.la3d_version() == 2 and re.search(r"#define\s+LA3D_ABI_VERSION\s+2\b", hdr)
    assert C.sizeof(_lib.FitArgs) == 232 and _lib.FitArgs._fields_[-1][0] == "method"
    import labelany3d_amd as la
    for fn in ("pack_label_bits", "fit_instances_labels", "label_instances", "LabelBits"):
        assert callable(getattr(la, fn)) and fn in la.__all__
    assert la.LabelBits._fields == ("bits", "image_index", "area")


def test_python_argument_errors_before_any_device_work():
    import labelany3d_amd as la

    lab = np.zeros((2, 8, 32), np.uint8)
    ids = [[1], [2, 3]]
    for bad in (lab.astype(np.float32), lab.astype(np.int64), lab.astype(bool), lab.astype(np.uint32)):
        with pytest.raises(ValueError, match="uint8, uint16, int16"):
            la.pack_label_bits(bad, ids)
    for bad in (np.zeros(32, np.uint8), np.zeros((1, 2, 8, 32), np.uint8)):
        with pytest.raises(ValueError, match=r"\(P,H,W\) or \(H,W\)"):
            la.pack_label_bits(bad, [[1]])
    for bad in (lab, np.zeros((2, 8, 32, 4), np.uint8), np.zeros((8, 3), np.uint8), np.zeros((1, 2, 8, 32, 3), np.uint8)):
        with pytest.raises(ValueError, match="rgb=True"):
            la.pack_label_bits(bad, ids, rgb=True)
    with pytest.raises(ValueError, match="rgb=True"):
        la.pack_label_bits(np.zeros((2, 8, 32, 3), np.int32), ids, rgb=True)
    for bad in ([[1]], [[1], [2], [3]], []):
        with pytest.raises(ValueError, match="one id sequence per image"):
            la.pack_label_bits(lab, bad)
    with pytest.raises(ValueError, match="one id sequence per image"):
        la.pack_label_bits(lab[0], ids)                       # (H,W) is one image
    with pytest.raises(ValueError, match="one id sequence per image"):
        la.pack_label_bits(np.zeros((8, 32, 3), np.uint8), ids, rgb=True)
    three = np.array([1, 2, 3], np.int32)
    for off in ([1, 1, 3], [0, 2, 1], [0, 1, 2], [0, 1, 4], [0, 3]):
        with pytest.raises(ValueError, match="inst_offsets"):
            la.pack_label_bits(lab, (three, np.asarray(off)))
    with pytest.raises(ValueError, match="int32"):
        la.pack_label_bits(lab.astype(np.int32), [[2**31], []])
    # the fit entry: the method / height rule first, then the packer's checks
    d, K = np.zeros((2, 8, 32), np.float32), np.eye(3)
    with pytest.raises(ValueError, match=MSG):
        la.fit_instances_labels(d, lab, ids, K, method="obb")
    with pytest.raises(ValueError, match="height_rule"):
        la.fit_instances_labels(d, lab, ids, K, height_rule="tallest")
    with pytest.raises(ValueError, match="one id sequence per image"):
        la.fit_instances_labels(d, lab, [[1]], K)
    with pytest.raises(ValueError, match="uint8, uint16, int16"):
        la.fit_instances_labels(d, lab.astype(np.float64), ids, K)
    with pytest.raises(ValueError, match="uint8, uint16, int16"):
        la.label_instances(lab.astype(np.float32))
    with pytest.raises(ValueError, match="rgb=True"):
        la.label_instances(lab, rgb=True)


def test_label_instances_on_the_host():
    """``label_instances`` runs where the labels lie: a NumPy map never needs the device"""
    import labelany3d_amd as la

    rs = np.random.RandomState(0)
    lab = rs.choice(np.array([0, 3, 7, 65535, 256], np.uint16), (2, 9, 13), p=[0.3, 0.3, 0.2, 0.15, 0.05])
    ids, areas = la.label_instances(lab, ignore=(0,), min_area=4)
    for p in range(2):
        u, c = np.unique(lab[p], return_counts=True)
        keep = (u != 0) & (c >= 4)
        np.testing.assert_array_equal(ids[p], u[keep])
        np.testing.assert_array_equal(areas[p], c[keep])
        assert ids[p].dtype == np.int32
    neg = np.array([[-5, -5, 7, 2**31 - 1], [-2**31, 0, 0, 7]], np.int32)
    ids, areas = la.label_instances(neg, ignore=())
    np.testing.assert_array_equal(ids[0], [-2**31, -5, 0, 7, 2**31 - 1])
    np.testing.assert_array_equal(areas[0], [1, 2, 2, 2, 1])


def test_c_entry_argument_errors_without_a_device():
    from labelany3d_amd import _lib

    L = _lib.lib
    one = (C.c_double * 64)()
    p = C.addressof(one)
    assert p % 4 == 0

    def call(labels=p, dtype=0, stride=256, P=1, H=8, W=32, W_out=32, off=p, lab=p, B=1, bits=p, bstride=8, area=p):
        return L.la3d_pack_label_bits(labels, dtype, stride, P, H, W, W_out, off, lab, B, bits, bstride, area, None)

    def refused(rc, *words):
        err = L.la3d_last_error()
        assert rc == -1 and b"la3d_pack_label_bits" in err, (rc, err)
        for w in words:
            assert w in err, err

    for dtype in (4, -1, 17):
        refused(call(dtype=dtype), b"dtype")
    refused(call(W_out=31), b"W_out")
    refused(call(B=-1))
    refused(call(P=-1))
    refused(call(H=0))
    refused(call(W=-3, W_out=-3))
    refused(call(stride=255), b"stride")
    refused(call(dtype=3, stride=255), b"stride")                  # RGB8: the stride counts pixels
    refused(call(bstride=7), b"bits_plane_stride")
    refused(call(W_out=64, bstride=15), b"bits_plane_stride")
    refused(call(H=7, W=45, W_out=45, stride=315, bstride=9), b"bits_plane_stride")   # needs ceil(315 / 32) = 10
    refused(call(bits=p + 1), b"aligned")
    refused(call(bits=p + 2), b"aligned")
    refused(call(labels=p + 1, dtype=1), b"aligned")
    refused(call(labels=p + 2, dtype=2), b"aligned")
    for null in ("labels", "off", "lab", "bits"):
        refused(call(**{null: None}), b"NULL")
    # nothing to do: success without touching a pointer (and without a device)
    assert call(B=0, labels=None, off=None, lab=None, bits=None, area=None, stride=0, bstride=0) == 0
    assert call(P=0, B=0, labels=None, off=None, lab=None, bits=None, area=None, stride=0, bstride=0) == 0
    assert call(P=0, labels=None, off=None, lab=None, bits=None, area=None) == 0
    for dtype in range(4):
        assert call(dtype=dtype, B=0) == 0
    refused(call(B=0, dtype=4), b"dtype")                          # (the dtype and the sizes are checked whatever B is)
    refused(call(B=0, W_out=31), b"W_out")
