"""CPU-only tests of the frames form of morphology on bit planes (include/la3d.h "morphology on bit planes", la3d_open_bits_frames): the
condition on the shared case list, the names on every layer, the C entry's refusals before any launch (fake pointers: nothing here
reaches a device), the workspace size, the Python argument errors, and the host arithmetic of the scaled table and the layouts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import open_bits_cases as OC
from . import open_bits_frames_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2


def test_the_case_list_exercises_the_opening():
    """at least half of all planes come back neither empty nor equal to their upscale (137 of 216 when the list was made); the 24 planes
    of k = 3, s = 4 are unchanged by construction - a x4 upscale is a union of 4 x 4 blocks"""
    assert len(FC.SIZES) == 12 and len(FC.IMAGE_INDEX) == 24
    changed = total = 0
    for k in FC.KS:
        for s in FC.SCALES:
            here = 0
            for m, p in zip(FC.planes(k, s), FC.IMAGE_INDEX):
                assert m.shape == FC.SIZES[p]
                want = OC.opening(m, k, s)
                here += bool(want.any()) and not np.array_equal(want, OC.upscale(m, s))
                total += 1
            assert (k, s) != (3, 4) or here == 0
            changed += here
    assert total == 216 and 2 * changed >= total, (changed, total)


def test_names_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _lib, frames, morph

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    assert re.search(r"\bsize_t la3d_open_bits_frames_workspace_bytes\s*\(", hdr) and re.search(r"\bint la3d_open_bits_frames\s*\(", hdr)
    for fn in ("la3d_open_bits_frames", "la3d_open_bits_frames_workspace_bytes"):
        assert fn in _lib.EXPORTS and hasattr(_lib.lib, fn), fn
    homes = dict(FrameGrid=frames, scaled_frames=frames, open_bits_frames=morph, bits_rects_frames=morph, select_crops_frames=morph)
    for fn, home in homes.items():   # (the frame table and its scaled form live in frames, morphology - both layouts - in morph)
        assert callable(getattr(la, fn)) and fn in la.__all__ and getattr(home, fn) is getattr(la, fn), fn
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2     # additive
    assert "last to first" in la.select_crops_frames.__doc__.lower() and "bboxes.json" in la.select_crops_frames.__doc__


class Fake:
    """fake "device" memory, 64-byte aligned: every call below is refused, or has nothing to do, before any launch"""

    def __init__(self):
        self.buf = (C.c_char * 32768)()
        self.p = (C.addressof(self.buf) + 63) & ~63


def call(f, **kw):
    from labelany3d_amd import _lib

    a = dict(bits=f.p, bits_words=64, offs=f.p + 2048, frames=f.p + 4096, P=2, H=8, W=32, ii=f.p + 6144, B=2, k=7, s=1, out=f.p + 8192,
             out_words=64, ooffs=f.p + 10240, stats=f.p + 12288, ws=f.p + 14336)
    a.update(kw)
    rc = _lib.lib.la3d_open_bits_frames(a["bits"], a["bits_words"], a["offs"], a["frames"], a["P"], a["H"], a["W"], a["ii"], a["B"], a["k"],
                                        a["s"], a["out"], a["out_words"], a["ooffs"], a["stats"], a["ws"], None)
    return rc, _lib.lib.la3d_last_error()


def test_c_entry_refuses_before_any_launch():
    f = Fake()
    for k in (0, 2, 6, 32, 33, -1, -7):
        rc, msg = call(f, k=k)
        assert rc == ARG and b"k must be" in msg, k
    for s in (0, 3, 5, 8, -1):
        rc, msg = call(f, s=s)
        assert rc == ARG and b"upscale must be" in msg, s
    assert call(f, out=None, stats=None)[0] == ARG                        # nothing to do
    for name in ("bits", "offs", "frames", "ii"):                         # a NULL that is needed
        assert call(f, **{name: None})[0] == ARG, name
    assert call(f, ooffs=None)[0] == ARG and call(f, ws=None)[0] == ARG
    assert call(f, B=-1)[0] == ARG and call(f, P=-1)[0] == ARG
    assert call(f, H=0)[0] == ARG and call(f, W=0)[0] == ARG and call(f, H=-3)[0] == ARG
    assert call(f, bits=f.p + 4)[0] == ARG and call(f, bits=f.p + 8)[0] == ARG          # 16 bytes
    assert call(f, out=f.p + 8192 + 4)[0] == ARG and call(f, out=f.p + 8192 + 8)[0] == ARG
    assert call(f, offs=f.p + 2048 + 4)[0] == ARG and call(f, ooffs=f.p + 10240 + 4)[0] == ARG and call(f, frames=f.p + 4096 + 4)[0] == ARG   # 8 bytes
    assert call(f, stats=f.p + 12288 + 2)[0] == ARG and call(f, ws=f.p + 14336 + 2)[0] == ARG and call(f, ii=f.p + 6144 + 2)[0] == ARG      # 4 bytes
    assert call(f, bits_words=-1)[0] == ARG and call(f, out_words=-1)[0] == ARG


def test_c_entry_rules_hold_for_an_empty_batch():
    f = Fake()
    assert call(f, B=0, k=4)[0] == ARG and call(f, B=0, s=3)[0] == ARG
    assert call(f, B=0, out=None, stats=None)[0] == ARG
    assert call(f, B=0, P=-1)[0] == ARG and call(f, B=0, H=0)[0] == ARG and call(f, B=0, W=0)[0] == ARG
    assert call(f, B=0, bits=f.p + 4)[0] == ARG and call(f, B=0, ii=f.p + 6144 + 2)[0] == ARG and call(f, B=0, offs=f.p + 2048 + 4)[0] == ARG
    assert call(f, B=0, bits_words=-1)[0] == ARG and call(f, B=0, out_words=-1)[0] == ARG
    assert call(f, B=0, out=f.p)[0] == ARG                                # in place
    assert call(f, B=0, W=8224)[0] == UNSUPPORTED
    # a valid empty batch is success without a launch, whatever the pointers; so is one without images
    assert call(f, B=0)[0] == 0 and call(f, B=0, P=0)[0] == 0
    assert call(f, B=0, bits=None, offs=None, frames=None, ii=None, ooffs=None, ws=None)[0] == 0
    assert call(f, B=0, out=None, ooffs=None)[0] == 0 and call(f, B=0, stats=None, ws=None)[0] == 0


def test_c_entry_refuses_overlapping_buffers():
    f = Fake()
    assert call(f, out=f.p)[0] == ARG                                    # in place
    assert call(f, out=f.p + 4 * 60)[0] == ARG                           # the last words of the input range
    assert call(f, bits=f.p + 8192 + 4 * 60)[0] == ARG                   # the input begins inside the output range
    assert call(f, bits_words=4096, out=f.p + 8192)[0] == ARG            # a long input buffer that holds the output
    rc, msg = call(f, out=f.p + 16)
    assert rc == ARG and b"overlap" in msg
    assert call(f, out=f.p + 256, B=0)[0] == 0                           # side by side: [p, p + 256) and [p + 256, p + 512)


def test_c_entry_unsupported_sizes():
    f = Fake()
    assert call(f, W=8224)[0] == UNSUPPORTED                              # upscale * W > 8192
    assert call(f, W=4128, s=2)[0] == UNSUPPORTED and call(f, W=2080, s=4)[0] == UNSUPPORTED
    assert call(f, H=(1 << 15) + 1, W=8192)[0] == UNSUPPORTED             # upscale * H * roundup32(upscale * W) > 2^28
    assert call(f, H=(1 << 21) + 1, s=4, W=1)[0] == UNSUPPORTED           # 4 H rows of 32 columns
    assert call(f, H=1 << 21, s=4, W=1, B=0)[0] == 0
    assert call(f, H=(1 << 26) + 1, s=4, W=32)[0] == UNSUPPORTED
    assert call(f, B=0x7fffffff, H=65, W=32)[0] == UNSUPPORTED            # B * bands > 2^31 - 1 (65 rows: two bands under any plan)


def test_workspace_bytes_is_monotone_and_zero_on_empty_input():
    from labelany3d_amd import _lib

    ws = _lib.lib.la3d_open_bits_frames_workspace_bytes
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
    # one record of 8 ints per band of the bounds, and no plan has bands of fewer than 32 rows
    assert ws(5, 140, 4) >= 5 * ((4 * 140 + 31) // 32) * 8 * 4


def host_grid(sizes):
    import torch

    import labelany3d_amd as la
    from labelany3d_amd.frames import _bounds, frame_table, table_words

    t = frame_table(list(sizes))
    return la.FrameGrid(torch.as_tensor(table_words(t)), t, *_bounds(t), [tuple(s) for s in sizes])


def host_bits(grid, ii):
    import torch

    import labelany3d_amd as la

    offs, total = la.frame_bits_offsets(grid.table_host, ii)
    return la.FrameBits(torch.zeros(max(total, 4), dtype=torch.int32), torch.as_tensor(offs), torch.as_tensor(np.asarray(ii, np.int32)),
                        torch.zeros(len(ii), dtype=torch.int32), grid.table_host, grid.H, grid.W)


def test_python_argument_errors_come_before_any_device_work():
    import labelany3d_amd as la

    grid = host_grid(FC.SIZES)                                            # on the host: never reaches a device
    fb = host_bits(grid, FC.IMAGE_INDEX)
    for k in (0, 2, 8, 33, -3, 7.0, True, "7"):
        with pytest.raises(ValueError, match="k must be"):
            la.open_bits_frames(grid, fb, k=k)
        with pytest.raises(ValueError, match="k must be"):
            la.select_crops_frames(grid, fb, k=k)
    for s in (0, 3, 8, -1, 2.0, True):
        with pytest.raises(ValueError, match="upscale must be"):
            la.open_bits_frames(grid, fb, upscale=s)
        with pytest.raises(ValueError, match="upscale must be"):
            la.select_crops_frames(grid, fb, upscale=s)
        with pytest.raises(ValueError, match="upscale must be"):
            la.scaled_frames(grid, s)
    other = host_grid(FC.SIZES[:-1] + ((32, 161),))
    for fn in (la.open_bits_frames, la.bits_rects_frames, la.select_crops_frames):
        with pytest.raises(ValueError, match="another frame table"):
            fn(other, fb)
        with pytest.raises(ValueError, match="must be the FrameBits"):
            fn(grid, (fb.bits, fb.offsets))
        with pytest.raises(ValueError, match="must be the FrameBits"):
            fn(grid, la.MaskBits(fb.bits.view(1, -1), 8, 32, 32))
        with pytest.raises(ValueError, match="frames must be"):
            fn(grid.table_host, fb)
    with pytest.raises(ValueError, match="min_area"):
        la.select_crops_frames(grid, fb, min_area=-1)
    with pytest.raises(ValueError, match="crop_size"):
        la.select_crops_frames(grid, fb, crop_size=0)
    with pytest.raises(ValueError, match="image_index"):
        la.open_bits_frames(grid, fb, image_index=FC.IMAGE_INDEX[:-1])
    with pytest.raises(ValueError, match="image_index"):
        la.open_bits_frames(grid, fb, image_index=np.full(24, 12))
    with pytest.raises(ValueError, match="image_index"):
        la.open_bits_frames(grid, fb, image_index=FC.IMAGE_INDEX.astype(np.float32))
    with pytest.raises(ValueError, match="overlaps"):
        la.open_bits_frames(grid, fb, out=fb.bits)
    with pytest.raises(ValueError, match="overlaps"):
        la.open_bits_frames(grid, fb, image_index=FC.IMAGE_INDEX, out=fb.bits[4:])
    for fn in (la.open_bits_frames, la.bits_rects_frames, la.select_crops_frames):
        with pytest.raises(ValueError, match="on the GPU"):
            fn(grid, fb)                                                  # the last check of all: where the planes live


def test_scaled_frames_is_the_frame_table_of_the_scaled_sizes():
    import labelany3d_amd as la
    from labelany3d_amd.frames import frame_table, table_words

    grid = host_grid(FC.SIZES)
    for s in (1, 2, 4):
        g = la.scaled_frames(grid, s, device="cpu")
        sizes = [(s * h, s * w) for h, w in FC.SIZES]
        want = frame_table(sizes)
        assert isinstance(g, la.FrameGrid) and g.sizes == sizes
        np.testing.assert_array_equal(g.table_host, want)
        np.testing.assert_array_equal(g.table.numpy(), table_words(want))
        assert (g.H, g.W) == (s * 140, OC.padded(s * 224))
        assert (g.table_host["W"] == [OC.padded(s * w) for _, w in FC.SIZES]).all() and (g.table_host["frame_width"] == [s * w for _, w in FC.SIZES]).all()
    np.testing.assert_array_equal(la.scaled_frames(grid, 1, device="cpu").table_host, grid.table_host)
    # the bounds are those of the scaled table, not the scaled bounds: 33 columns are stored 64 wide, 132 columns 160 wide
    g = la.scaled_frames(host_grid([(8, 33), (2, 5)]), 4, device="cpu")
    assert (g.H, g.W) == (32, 160)
    assert la.scaled_frames(host_grid([]), 2, device="cpu").sizes == []


def test_the_compact_layout_is_frame_bits_offsets_of_the_scaled_table():
    """the host arithmetic ``open_bits_frames`` lays its planes out with (the device test compares the offsets it returns)"""
    import labelany3d_amd as la

    grid = host_grid(FC.SIZES)
    for s in (1, 2, 4):
        offs, total = la.frame_bits_offsets(la.scaled_frames(grid, s, device="cpu").table_host, FC.IMAGE_INDEX)
        words = [FC.plane_words(s * FC.SIZES[p][0], s * FC.SIZES[p][1]) for p in FC.IMAGE_INDEX]
        step = [(w + 3) // 4 * 4 for w in words]
        assert offs.tolist() == np.concatenate([[0], np.cumsum(step)[:-1]]).tolist() and total == sum(step)
        assert (offs % 4 == 0).all()
