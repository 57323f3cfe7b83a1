"""CPU-only tests of crop-space masks as bit planes (include/la3d.h "crop-space masks as bit planes"): the NumPy restatement of the
rule against what the reference's own ``restore_mask_from_crop`` gave (tests/golden/g18_crops.npz), the host arithmetic of
``crop_placement``, the names on every layer, and the C entries' refusals before any launch (fake pointers: nothing here reaches a
device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import crop_bits_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_C = ("la3d_pack_crop_bits", "la3d_pack_crop_bits_frames")
ARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def g():
    return CC.load_golden()


def test_fixture_holds_the_cases_it_must(g):
    sides, raised, par, fr = g["side"], g["raised"], g["params"], g["frame"]
    assert len(sides) == len(CC.fixture_cases()) and (g["crops"] == CC.fixture_crops()).all()
    np.testing.assert_array_equal(g["shapes"], CC.FRAMES)
    for f, (H, W) in enumerate(CC.FRAMES):
        s, p = sides[fr == f], par[fr == f]
        assert (s > CC.S_FIX).any() and ((s < CC.S_FIX) & (s > 1)).any() and (s == CC.S_FIX).any() and (s == 1).any() and (s == 0).any()
        half = p[:, 0] % 1 == 0.5
        assert (np.floor(p[half, 0]) % 2 == 0).any() and (np.floor(p[half, 0]) % 2 == 1).any()
        assert {-2.5, -3.5} <= set(p[:, 0]) and {-2.5, -3.5} <= set(p[:, 1])
        x1, y1 = g["xy1"][fr == f].T
        x2, y2 = x1 + s, y1 + s
        inside = (x2 > 0) & (x1 < W) & (y2 > 0) & (y1 < H) & (s > 0)
        for over in (x1 < 0, y1 < 0, x2 > W, y2 > H, (x1 < 0) & (y1 < 0), (x2 > W) & (y2 > H)):     # four borders, two corners
            assert (inside & over).any()
        for out in (x2 <= 0, x1 >= W, y2 <= 0, y1 >= H):                                                # wholly outside, each side
            assert ((s > 0) & out).any()
    assert raised.any() and not raised.all()
    assert len(g["side_table"]) == 1024 and (g["side_table"] != np.arange(1, 1025)).any()   # int(256 / (256 / k)) is not always k


def test_restatement_equals_the_reference_on_every_case(g):
    """the cases in which the reference raised included: there the restatement gives an empty mask"""
    masks = CC.golden_masks(g)
    for name, f, p, crop, raised, want in zip(g["names"], g["frame"], g["params"], g["crops"], g["raised"], masks):
        got = CC.restore(crop, p[0], p[1], p[2], CC.FRAMES[f])
        assert got.dtype == bool and got.shape == CC.FRAMES[f]
        np.testing.assert_array_equal(got, want, err_msg=str(name))
        if raised:
            assert not got.any(), name
    assert sum(int(m.sum()) for m in masks) > 10000


def test_every_raised_case_is_one_of_the_two_documented(g):
    for name, f, s, (x1, y1), raised in zip(g["names"], g["frame"], g["side"], g["xy1"], g["raised"]):
        H, W = CC.FRAMES[f]
        outside = x1 + s <= 0 or x1 >= W or y1 + s <= 0 or y1 >= H
        if raised:
            assert s <= 0 or outside, name


def test_crop_placement_is_the_reference_arithmetic(g):
    from labelany3d_amd import crop_placement

    place = crop_placement(g["params"], CC.S_FIX)
    assert place.dtype == np.int32 and place.shape == (len(g["params"]), 4)
    np.testing.assert_array_equal(place[:, 2], g["side"])
    np.testing.assert_array_equal(place[:, :2], g["xy1"])
    assert (place[:, 3] == 0).all()
    k = np.arange(1, 1025)
    table = crop_placement([(0.0, 0.0, 256 / int(i)) for i in k], 256)
    np.testing.assert_array_equal(table[:, 2], g["side_table"])
    # half to even, lists and arrays alike; values beyond int32 are clamped, not wrapped
    np.testing.assert_array_equal(crop_placement([(0.5, 1.5, 1.0), (-0.5, -1.5, 2.0), (2.5, -2.5, 0.5)], 16)[:, :3],
                                  [[0, 2, 16], [0, -2, 8], [2, -2, 32]])
    big = crop_placement(np.array([[1e12, -1e12, 1e-12]]), 16)
    np.testing.assert_array_equal(big[0, :3], [2 ** 31 - 1, -(2 ** 31 - 1), 2 ** 31 - 1])
    assert crop_placement(np.zeros((0, 3)), 16).shape == (0, 4)
    with pytest.raises(ValueError):
        crop_placement([(1.0, 2.0)], 16)


def test_names_on_every_layer_and_the_shim_keeps_the_reference(tmp_path, monkeypatch):
    import labelany3d_amd as la
    from labelany3d_amd import _lib, frames, masks
    from labelany3d_amd import util as impl_util

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    for fn in NEW_C:
        assert re.search(rf"\bint {fn}\s*\(", hdr), fn
        assert fn in _lib.EXPORTS and hasattr(_lib.lib, fn), fn
    assert "crop-space masks as bit planes" in hdr
    for fn in ("crop_placement", "pack_crop_bits", "pack_crop_bits_frames"):
        assert callable(getattr(la, fn)) and fn in la.__all__ and getattr(masks, fn) is getattr(la, fn), fn
    assert frames.pack_crop_bits_frames is la.pack_crop_bits_frames
    assert callable(impl_util.restore_mask_from_crop)
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2     # additive
    # `from util import restore_mask_from_crop` through the shim still resolves to the reference's own function
    import sys

    import labelany3d_amd.compat as compat

    ref = tmp_path / "ref"
    ref.mkdir()
    (ref / "util.py").write_text("def depth_to_points(*a, **k):\n    return 'reference'\n\ndef restore_mask_from_crop(*a):\n    return 'ref-restore'\n")
    shim_dir = os.path.dirname(os.path.abspath(compat.__file__))
    monkeypatch.setattr(sys, "path", [shim_dir, str(ref)] + [p for p in sys.path if p not in (shim_dir, str(ref))])
    monkeypatch.setattr(compat, "_loaded", {})
    held = sys.modules.pop("util", None)
    try:
        ns = {}
        exec("from util import restore_mask_from_crop, depth_to_points", ns)
        assert ns["restore_mask_from_crop"]() == "ref-restore" and ns["depth_to_points"] is impl_util.depth_to_points
    finally:
        sys.modules.pop("util", None)
        if held is not None:
            sys.modules["util"] = held
    assert "restore_mask_from_crop" not in compat._HOT["util"]


class Fake:
    """fake "device" memory, 64-byte aligned: every call below is refused, or has nothing to do, before any launch"""

    def __init__(self):
        self.buf = (C.c_char * 8192)()
        self.p = (C.addressof(self.buf) + 63) & ~63


def uniform_call(f, **kw):
    from labelany3d_amd import _lib

    a = dict(crops=f.p, cs=256, pitch=16, step=1, S=16, thr=0, place=f.p + 1024, B=2, H=8, W=32, W_out=32, bits=f.p + 2048, stride=8,
             area=f.p + 3072)
    a.update(kw)
    rc = _lib.lib.la3d_pack_crop_bits(a["crops"], a["cs"], a["pitch"], a["step"], a["S"], a["thr"], a["place"], a["B"], a["H"], a["W"], a["W_out"],
                                      a["bits"], a["stride"], a["area"], None)
    return rc, _lib.lib.la3d_last_error()


def frames_call(f, **kw):
    from labelany3d_amd import _lib

    a = dict(crops=f.p, cs=256, pitch=16, step=1, S=16, thr=0, place=f.p + 1024, frames=f.p + 1536, P=1, H=8, W=32, ii=f.p + 2048, B=2,
             bits=f.p + 3072, offs=f.p + 2560, area=f.p + 3584)
    a.update(kw)
    rc = _lib.lib.la3d_pack_crop_bits_frames(a["crops"], a["cs"], a["pitch"], a["step"], a["S"], a["thr"], a["place"], a["frames"], a["P"], a["H"],
                                             a["W"], a["ii"], a["B"], a["bits"], a["offs"], a["area"], None)
    return rc, _lib.lib.la3d_last_error()


SOURCE_REFUSALS = [dict(S=0), dict(S=-3), dict(step=0), dict(pitch=15), dict(pitch=63, step=4), dict(thr=-1), dict(thr=256), dict(cs=255),
                   dict(cs=15 * 64 + 15 * 4, pitch=64, step=4)]


@pytest.mark.parametrize("call", [uniform_call, frames_call], ids=["uniform", "frames"])
def test_c_entries_refuse_before_any_launch(call):
    f = Fake()
    for kw in SOURCE_REFUSALS:
        assert call(f, **kw)[0] == ARG, kw
        assert call(f, B=0, **kw)[0] == ARG, kw                     # the source's rules hold for an empty batch too
    assert call(f, cs=15 * 64 + 15 * 4 + 1, pitch=64, step=4, B=0)[0] == 0     # exactly a crop of RGBA alpha
    assert call(f, B=0)[0] == 0 and call(f, B=0, crops=None, place=None, bits=None)[0] == 0
    assert call(f, B=-1)[0] == ARG and call(f, H=0)[0] == ARG and call(f, W=0)[0] == ARG
    assert call(f, crops=None)[0] == ARG and call(f, place=None)[0] == ARG and call(f, bits=None)[0] == ARG
    assert call(f, place=f.p + 1026)[0] == ARG and call(f, area=f.p + 3586)[0] == ARG
    assert call(f, H=1025, W=1024, **({"W_out": 1024, "stride": 1 << 20} if call is uniform_call else {}))[0] == UNSUPPORTED


def test_uniform_refusals_are_those_of_the_run_length_packer():
    f = Fake()
    assert uniform_call(f, W_out=31)[0] == ARG                       # W_out < W
    assert uniform_call(f, W=30, W_out=31)[0] == ARG                 # padded, but to no multiple of 32
    assert uniform_call(f, stride=7)[0] == ARG                       # a plane stride smaller than a plane
    assert uniform_call(f, bits=f.p + 2050)[0] == ARG                # bits not 4-byte aligned


def test_frames_refusals_are_those_of_the_run_length_packer():
    f = Fake()
    assert frames_call(f, P=-1)[0] == ARG
    assert frames_call(f, bits=f.p + 3076)[0] == ARG                 # bits not 16-byte aligned
    assert frames_call(f, frames=None)[0] == ARG and frames_call(f, ii=None)[0] == ARG and frames_call(f, offs=None)[0] == ARG
    assert frames_call(f, offs=f.p + 2564)[0] == ARG                 # bits_offsets not 8-byte aligned


def test_python_argument_errors_come_before_any_device_work():
    import torch

    import labelany3d_amd as la

    crops = np.zeros((2, 16, 16), np.uint8)
    par = [(0.0, 0.0, 1.0)] * 2
    dev = torch.device("cuda", 0)     # (never touched: every call below raises first)
    with pytest.raises(ValueError, match="empty frame"):
        la.pack_crop_bits(crops, par, (0, 8), device=dev)
    with pytest.raises(ValueError, match="area must be"):
        la.pack_crop_bits(crops, par, (32, 8), device=dev, area=np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="frames must be"):
        la.pack_crop_bits_frames(None, crops, par, [0, 0])
