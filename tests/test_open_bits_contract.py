"""CPU-only tests of morphology on bit planes (include/la3d.h "morphology on bit planes"): the NumPy restatement of the opening against
what SciPy gave (tests/golden/g19_opening.npz) and gives (where it imports), the names on every layer, the C entry's refusals before
any launch (fake pointers: nothing here reaches a device), the workspace size, and the host arithmetic of ``crop_params``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import open_bits_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def g():
    return OC.load_golden()


def test_restatement_equals_the_fixture(g):
    """always: what SciPy gave when the fixture was made; and the condition on the fixture - at least half of its planes come back
    neither empty nor unchanged"""
    cases = OC.fixture_cases()
    np.testing.assert_array_equal(g["cases"], cases)
    np.testing.assert_array_equal(g["shapes"], OC.FRAMES)
    changed = total = 0
    for i, ((f, k, s), planes) in enumerate(zip(cases, OC.fixture_planes())):
        ins, outs = OC.golden_case(g, i)
        np.testing.assert_array_equal(ins, planes)
        for m, want in zip(ins, outs):
            np.testing.assert_array_equal(OC.opening(m, k, s), want, err_msg=f"case {i}: frame {f}, k {k}, s {s}")
            changed += bool(want.any()) and not np.array_equal(want, OC.upscale(m, s))
            total += 1
    assert total == 108 and 2 * changed >= total, (changed, total)
    assert os.path.getsize(OC.GOLDEN) < 110 * 1024


def test_restatement_equals_scipy_on_random_cases():
    ndi = pytest.importorskip("scipy.ndimage")
    cases = OC.random_cases(1907, 200)
    assert {c[1] for c in cases} == {1, 3, 5, 7, 9, 15, 31} and {c[2] for c in cases} == {1, 2, 4}
    bad = [i for i, (m, k, s) in enumerate(cases)
           if not np.array_equal(OC.opening(m, k, s), ndi.binary_opening(OC.upscale(m, s), np.ones((k, k))))]
    assert not bad, bad


def test_names_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _lib, masks

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    assert "morphology on bit planes" in hdr
    assert re.search(r"\bsize_t la3d_open_bits_workspace_bytes\s*\(", hdr) and re.search(r"\bint la3d_open_bits\s*\(", hdr)
    for fn in ("la3d_open_bits", "la3d_open_bits_workspace_bytes"):
        assert fn in _lib.EXPORTS and hasattr(_lib.lib, fn), fn
    for fn in ("open_bits", "bits_rects", "crop_params", "select_crops"):
        assert callable(getattr(la, fn)) and fn in la.__all__ and getattr(masks, fn) is getattr(la, fn), fn
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2     # additive
    assert "last to first" in la.select_crops.__doc__.lower() and "bboxes.json" in la.select_crops.__doc__


class Fake:
    """fake "device" memory, 64-byte aligned: every call below is refused, or has nothing to do, before any launch"""

    def __init__(self):
        self.buf = (C.c_char * 16384)()
        self.p = (C.addressof(self.buf) + 63) & ~63


def call(f, **kw):
    from labelany3d_amd import _lib

    a = dict(bits=f.p, stride=8, B=2, H=8, W=32, fw=32, k=7, s=1, out=f.p + 4096, ostride=8, W_out=32, stats=f.p + 8192, ws=f.p + 12288)
    a.update(kw)
    rc = _lib.lib.la3d_open_bits(a["bits"], a["stride"], a["B"], a["H"], a["W"], a["fw"], a["k"], a["s"], a["out"], a["ostride"], a["W_out"],
                                 a["stats"], a["ws"], None)
    return rc, _lib.lib.la3d_last_error()


def test_c_entry_refuses_before_any_launch():
    f = Fake()
    for k in (0, 2, 6, 32, 33, -1, -7):
        assert call(f, k=k)[0] == ARG, k
    for s in (0, 3, 5, 8, -1):
        assert call(f, s=s)[0] == ARG, s
    assert call(f, fw=0)[0] == ARG and call(f, fw=33)[0] == ARG and call(f, fw=-1)[0] == ARG
    assert call(f, W_out=31)[0] == ARG                                   # W_out < s * frame_width
    assert call(f, s=2, W_out=63, ostride=32)[0] == ARG
    assert call(f, stride=7)[0] == ARG and call(f, ostride=7)[0] == ARG    # a stride shorter than its plane
    assert call(f, s=4, W_out=128, ostride=127)[0] == ARG                # 32 rows of 128: 128 words
    assert call(f, bits=None)[0] == ARG and call(f, ws=None)[0] == ARG    # a NULL that is needed
    assert call(f, out=None, stats=None)[0] == ARG                       # nothing to do
    assert call(f, B=-1)[0] == ARG and call(f, H=0)[0] == ARG and call(f, W=0)[0] == ARG
    assert call(f, bits=f.p + 2)[0] == ARG and call(f, out=f.p + 4098)[0] == ARG and call(f, stats=f.p + 8194)[0] == ARG
    # the rules hold for an empty batch too; a valid empty batch is success without a launch, whatever the pointers
    assert call(f, B=0, k=4)[0] == ARG and call(f, B=0, s=3)[0] == ARG and call(f, B=0, fw=40)[0] == ARG
    assert call(f, B=0)[0] == 0 and call(f, B=0, bits=None, out=None, ws=None)[0] == 0


def test_c_entry_refuses_overlapping_planes():
    f = Fake()
    assert call(f, out=f.p)[0] == ARG                                    # in place
    assert call(f, out=f.p + 4 * 15)[0] == ARG                           # the last word of the input range
    assert call(f, bits=f.p + 4096 + 4 * 15, stride=8)[0] == ARG         # the input begins inside the output range
    assert call(f, stride=600, out=f.p + 2048)[0] == ARG                 # long strides: planes of one lie between planes of the other
    rc, msg = call(f, out=f.p + 4)
    assert rc == ARG and b"overlap" in msg


def test_c_entry_unsupported_sizes():
    f = Fake()
    assert call(f, W=8224, fw=8193, W_out=8224, stride=1 << 20, ostride=1 << 20)[0] == UNSUPPORTED      # s * frame_width > 8192
    assert call(f, W=4128, fw=4097, s=2, W_out=8224, stride=1 << 20, ostride=1 << 20)[0] == UNSUPPORTED
    assert call(f, H=1 << 16, W=8192, fw=8192, W_out=8192, stride=1 << 30, ostride=1 << 30)[0] == UNSUPPORTED   # s * H * W_out > 2^28
    assert call(f, H=(1 << 26) + 1, s=4, W=1, fw=1, W_out=4, stride=1 << 30, ostride=1 << 30)[0] == UNSUPPORTED


def test_workspace_bytes_is_monotone_and_zero_on_empty_input():
    from labelany3d_amd import _lib

    ws = _lib.lib.la3d_open_bits_workspace_bytes
    assert ws(0, 480, 4) == 0 and ws(4, 0, 4) == 0 and ws(-1, 480, 4) == 0 and ws(4, -3, 1) == 0
    assert ws(1, 1, 1) > 0
    sizes = [ws(B, 480, 4) for B in (1, 2, 16, 300, 1024)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    for s in (1, 2, 4):
        sizes = [ws(3, H, s) for H in (1, 31, 32, 33, 480, 481, 4096, 1 << 20)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    for H in (1, 33, 480, 1 << 20):
        assert ws(3, H, 1) <= ws(3, H, 2) <= ws(3, H, 4)
    assert ws(1 << 20, 1 << 20, 4) > 1 << 32                              # size_t: no 32-bit wrap


CROP_LITERALS = [((40, 80, 400, 240), 571, (-11.375, -21.375, 3.586690017513135)),
                 ((0, 0, 7, 7), 10, (-0.375, -0.375, 204.8)),
                 ((13, 5, 101, 350), 500, (-46.625, -17.5, 4.096))]


def test_crop_params_against_literals_derived_by_hand():
    """reference src/util.py:142-157: side = int(max(w, h) / 0.7), offset = x + (w - side) / 2, scale = crop_size / side; then
    src/batch_scripts/get_crops_enhanced.py:98: offsets / 4, scale * 4"""
    from labelany3d_amd import crop_params

    stats = np.array([[9999, *r] for r, _, _ in CROP_LITERALS] + [[0, 0, 0, 0, 0]], np.int32)
    got = crop_params(stats, crop_size=512, upscale=4)
    assert got.dtype == np.float64 and got.shape == (4, 3)
    for row, (rect, side, want) in zip(got, CROP_LITERALS):
        assert int(max(rect[2], rect[3]) / 0.7) == side
        assert tuple(row) == want, (rect, tuple(row), want)
        assert list(row) == OC.crop_rule(*rect)
    assert np.isnan(got[3]).all()
    np.testing.assert_array_equal(crop_params(stats[:, 1:]), got)         # (B, 4): x, y, w, h
    assert crop_params(np.zeros((0, 5), np.int32)).shape == (0, 3)
    np.testing.assert_array_equal(crop_params(stats[:1], crop_size=256, upscale=1), [[40 + (400 - 571) / 2, 80 + (240 - 571) / 2, 256 / 571]])
    with pytest.raises(ValueError):
        crop_params(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        crop_params(stats, crop_size=0)


def test_crop_placement_of_crop_params_contains_the_rectangle():
    """the paste square ``restore_mask_from_crop`` fills for these parameters holds the rectangle, scaled back by the upscale"""
    from labelany3d_amd import crop_params, crop_placement

    rs = np.random.RandomState(5)
    x, y = rs.randint(0, 2000, 200), rs.randint(0, 1500, 200)
    w, h = rs.randint(32, 900, 200), rs.randint(32, 900, 200)
    stats = np.stack([w * h, x, y, w, h], 1).astype(np.int32)
    # side = int(max / 0.7) leaves (side - max) / 2 >= (0.4286 * 32 - 1) / 2 = 6.3 upscaled pixels beside the rectangle, at least 1.59
    # original pixels at upscale 4: more than the half pixel round() can move the corner plus the pixel int() can take off the side
    for S, up in ((512, 4), (256, 4), (512, 2), (512, 1)):
        place = crop_placement(crop_params(stats, crop_size=S, upscale=up), S)
        for (x1, y1, side, _), (_, rx, ry, rw, rh) in zip(place.tolist(), stats.tolist()):
            assert x1 <= rx // up and x1 + side >= -((rx + rw) // -up), (S, up, x1, side, rx, rw)
            assert y1 <= ry // up and y1 + side >= -((ry + rh) // -up), (S, up, y1, side, ry, rh)


def test_python_argument_errors_come_before_any_device_work():
    import torch

    import labelany3d_amd as la

    mb = la.MaskBits(torch.zeros((2, 8), dtype=torch.int32), 8, 32, 32)     # on the host: never reaches a device
    for k in (0, 2, 8, 33, -3, 7.0, True, "7"):
        with pytest.raises(ValueError, match="k must be"):
            la.open_bits(mb, k=k)
    for s in (0, 3, 8, -1, 2.0, True):
        with pytest.raises(ValueError, match="upscale must be"):
            la.open_bits(mb, upscale=s)
        with pytest.raises(ValueError, match="upscale must be"):
            la.select_crops(mb, upscale=s)
    with pytest.raises(ValueError, match="must be a MaskBits"):
        la.open_bits((mb.bits, 8, 32, 32))
    with pytest.raises(ValueError, match="must be a MaskBits"):
        la.bits_rects(mb.bits)
    with pytest.raises(ValueError, match="on the GPU"):
        la.open_bits(mb)
    with pytest.raises(ValueError, match="frame_width"):
        la.open_bits(la.MaskBits(mb.bits, 8, 32, 33))
    with pytest.raises(ValueError, match="min_area"):
        la.select_crops(mb, min_area=-1)
    with pytest.raises(ValueError, match="crop_size"):
        la.select_crops(mb, crop_size=0)
