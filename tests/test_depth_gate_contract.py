"""CPU-only tests of the depth gate on bit planes (include/la3d.h "depth gate on bit planes"): the NumPy restatement on hand-made
cases, the names on every layer, the layout of the argument block, the C entry's refusals before any launch (fake pointers: nothing
here reaches a device) and the Python argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import depth_gate_cases as DG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2
NAN, INF = float("nan"), float("inf")


def f32(*rows):
    return np.array(rows, np.float32)


def test_restatement_two_pixels_average_in_float32():
    keep, counts, levels = DG.gate(f32([1, 2, 5]), np.array([[True, True, False]]))
    assert levels.dtype == np.float32 and levels.tolist() == [1.5, 0.5, 2.25]
    assert counts.tolist() == [2, 2, 2] and keep.tolist() == [[True, True, False]]
    # the average of the two middle values is a float32 sum halved, not a float64 one rounded
    a, b = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    _, _, levels = DG.gate(f32([a, b]), np.ones((1, 2), bool))
    assert levels[0] == (a + b) / np.float32(2.0)


def test_restatement_one_ulp_off_a_constant_plane():
    d = np.full((4, 5), 2.0, np.float32)
    d[2, 3] = np.nextafter(np.float32(2.0), np.float32(3.0))
    m = np.ones((4, 5), bool)
    keep, counts, levels = DG.gate(d, m)                       # mad == 0: only the pixels AT the median stay
    assert levels.tolist() == [2.0, 0.0, 0.0] and counts.tolist() == [20, 20, 19] and not keep[2, 3] and keep.sum() == 19
    keep, counts, levels = DG.gate(d, m, min_band=0.01)        # the floor of the band keeps it
    assert levels.tolist() == [2.0, 0.0, float(np.float32(0.01))] and counts.tolist() == [20, 20, 20] and keep.all()


def test_restatement_invalid_and_fill_values():
    d = f32([2.0, NAN, INF, -INF, 2.1, 1.9, 10000.0, 2.05])
    m = np.ones((1, 8), bool)
    keep, counts, levels = DG.gate(d, m)
    assert counts.tolist() == [8, 5, 4]                        # NaN and +-inf are never valid; 10000.0 is valid and gated
    assert keep.tolist() == [[True, False, False, False, True, True, False, True]]
    assert levels[0] == np.float32(2.05)
    keep2, counts2, _ = DG.gate(d, m, far=9999.0)              # far handles the fill by itself
    assert counts2.tolist() == [8, 4, 4] and np.array_equal(keep2, keep)
    keep3, counts3, levels3 = DG.gate(d, m, near=5.0, far=6.0)  # an empty valid set
    assert not keep3.any() and counts3.tolist() == [8, 0, 0] and np.isnan(levels3).all() and levels3.dtype == np.float32
    _, counts4, levels4 = DG.gate(d, np.zeros((1, 8), bool))
    assert counts4.tolist() == [0, 0, 0] and np.isnan(levels4).all()
    # near / far are inclusive and k = 0 keeps the pixels at the median
    assert DG.gate(f32([1, 2, 3]), np.ones((1, 3), bool), near=1.0, far=3.0, k=0.0)[1].tolist() == [3, 3, 1]


def test_restatement_uniform_surface_keeps_every_pixel_at_default_k():
    d = np.linspace(1.0, 3.0, 1001, dtype=np.float32)[None]
    keep, counts, levels = DG.gate(d, np.ones_like(d, bool))
    assert keep.all() and counts.tolist() == [1001, 1001, 1001] and abs(levels[1] - 0.5) < 1e-3


def test_case_generators_cover_what_they_promise():
    for H, W, pad in DG.FRAMES:
        names, depths, masks = DG.planes(H, W)
        assert len(set(names)) == len(names) == len(depths) == len(masks) and depths.dtype == np.float32 and masks.dtype == bool
        by = dict(zip(names, masks))
        assert [int(by[f"smooth/{n}"].sum()) for n in ("empty", "one", "two", "full")] == [0, 1, 2, H * W]
        assert by["smooth/odd"].sum() % 2 == 1 and by["smooth/even"].sum() % 2 == 0 and by["smooth/even"].sum() > 2
        bad = depths[names.index("invalid/full")]
        assert np.isnan(bad).any() and (bad == np.inf).any() and (bad == -np.inf).any() and (bad == DG.FILL).any()
        assert (depths[names.index("negative/full")] < 0).all() and len({*np.sign(depths[names.index("mixed/full")]).ravel()}) >= 2
        assert len(np.unique(depths[names.index("ulps/full")].view(np.uint32) >> 4)) == 1
        gap = DG.not_image(H, W, DG.stored_width(W, pad))
        assert (np.unpackbits(gap.view(np.uint8)).sum() > 0) == (pad or (H * W) % 32 != 0)
        assert not (DG.pack(masks, DG.stored_width(W, pad)) & gap).any()
    names, depths, masks = DG.big_planes()
    counts = dict(zip(names, masks.reshape(len(masks), -1).sum(1)))
    assert depths.shape[1:] == DG.BIG == (96, 96) and counts["smooth"] == 9216 > 6144
    assert {counts[f"count_{c}"] for c in (6143, 6144, 6145, 6146)} == {6143, 6144, 6145, 6146}
    lv = dict(zip(names, depths))
    assert (lv["levels_50_50"] == 2.0).sum() == 4608 and (lv["levels_49_51"] == 2.0).sum() == 4516 and len(np.unique(lv["constant"])) == 1
    # near / far of PARAMS lie on either side of the smooth planes' median; min_band lies above and below k * mad
    med, mad, _ = DG.gate(lv["smooth"], masks[names.index("smooth")])[2]
    assert 2.3 < med < 2.7 and any(p.get("near", -INF) > med for p in DG.PARAMS) and any(-INF < p.get("near", -INF) < med for p in DG.PARAMS)
    assert any(p.get("far", INF) < med for p in DG.PARAMS) and any(med < p.get("far", INF) < INF for p in DG.PARAMS)
    assert any(p.get("k") == 0.0 for p in DG.PARAMS)
    assert any(p.get("min_band", 0) > p.get("k", 4.5) * mad for p in DG.PARAMS) and any(0 < p.get("min_band", 0) < p.get("k", 4.5) * mad for p in DG.PARAMS)
    depth, mask = DG.scene()
    keep, counts, levels = DG.gate(depth, mask)
    assert counts.tolist() == [1280, 1280, 1151] and abs(levels[0] - 2.0) < 0.05 and depth[keep].max() < 2.06 and levels[2] > 0.1


def test_names_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _build, _lib, bits, masks

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    assert "depth gate on bit planes" in hdr and re.search(r"\bint la3d_depth_gate_bits\s*\(const la3d_depth_gate_args\* args\)", hdr)
    assert "la3d_depth_gate_bits" in _lib.EXPORTS and hasattr(_lib.lib, "la3d_depth_gate_bits")
    for fn in ("gate_depth_bits", "depth_gate_stats", "DepthGateStats"):
        assert callable(getattr(la, fn)) and fn in la.__all__ and getattr(bits, fn) is getattr(la, fn) is getattr(masks, fn), fn
    assert la.DepthGateStats._fields == ("counts", "levels")
    assert any(s.endswith("la3d_depth_gate.hip") for s in _build.SOURCES) and any(h.endswith("la3d_select.hpp") for h in _build.HEADERS)
    assert "la3d_depth_gate.hip" in open(_build.__file__).read().split("SOURCES =")[0]      # its comment line
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2     # additive
    assert "min_band" in la.gate_depth_bits.__doc__ and "mad == 0" in la.gate_depth_bits.__doc__
    assert str(_lib.DEPTH_GATE_MAX_PIXELS) in hdr and _lib.DEPTH_GATE_MAX_PIXELS >= 819200


def test_block_layout_matches_the_header():
    """the ctypes block against the header's text: the same fields in the same order with the same types, the natural offsets, and
    the size the header states"""
    from labelany3d_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    stated, body = re.search(r"typedef struct la3d_depth_gate_args \{\s*/\* (\d+) bytes \*/(.*?)\} la3d_depth_gate_args;", hdr, re.S).groups()
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        base, star, names = m.group(1), m.group(2), m.group(3)
        for nm in names.split(","):
            want.append((nm.strip(), C.c_void_p if star else ctype[base]))
    assert [(n, t) for n, t in _lib.DepthGateArgs._fields_] == want
    off = 0
    for n, t in want:
        off = (off + C.alignment(t) - 1) // C.alignment(t) * C.alignment(t)
        assert getattr(_lib.DepthGateArgs, n).offset == off, n
        off += C.sizeof(t)
    assert C.sizeof(_lib.DepthGateArgs) == int(stated) == 120 == (off + 7) // 8 * 8
    assert _lib.DepthGateArgs.depth.offset == 40 and _lib.DepthGateArgs.stream.offset == 112


class Fake:
    """fake "device" memory, 64-byte aligned: every call below is refused, or has nothing to do, before any launch"""

    def __init__(self):
        self.buf = (C.c_char * 32768)()
        self.p = (C.addressof(self.buf) + 63) & ~63


def call(f, size=None, **kw):
    from labelany3d_amd import _lib

    a = dict(B=2, H=8, W=32, frame_width=0, k=4.5, min_band=0.0, near=-INF, far=INF, reserved=0,
             depth=f.p + 16384, depth_plane_stride=256, image_index=None, mask_bits=f.p, bits_plane_stride=8,
             out_bits=f.p + 4096, out_plane_stride=8, counts=f.p + 8192, levels=f.p + 12288, stream=None)
    a.update(kw)
    blk = _lib.DepthGateArgs(struct_size=C.sizeof(_lib.DepthGateArgs) if size is None else size, **a)
    rc = _lib.lib.la3d_depth_gate_bits(C.byref(blk))
    return rc, _lib.lib.la3d_last_error()


def refused(f, code, word, **kw):
    rc, msg = call(f, **kw)
    assert rc == code and word.encode() in msg and msg.startswith(b"la3d_depth_gate_bits: "), (kw, rc, msg)


def test_c_entry_refuses_before_any_launch():
    from labelany3d_amd import _lib

    f = Fake()
    for size in (0, 112, 119, 121, 128, -1):
        refused(f, ARG, "struct_size", size=size)
    assert _lib.lib.la3d_depth_gate_bits(None) == ARG and _lib.lib.la3d_last_error().startswith(b"la3d_depth_gate_bits: ")
    for kw in (dict(B=-1), dict(H=0), dict(W=0), dict(H=-3), dict(W=-1)):
        refused(f, ARG, "B >= 0, H, W > 0", **kw)
    for fw in (-1, 33, 1 << 20):
        refused(f, ARG, "frame_width", frame_width=fw)
    for v in (-1.0, -1e-30, NAN, INF, -INF):
        refused(f, ARG, "k must be", k=v)
        refused(f, ARG, "min_band must be", min_band=v)
    refused(f, ARG, "near and far", near=NAN)
    refused(f, ARG, "near and far", far=NAN)
    refused(f, ARG, "reserved", reserved=1)
    for v in (-1, 1, 255):
        refused(f, ARG, "depth_plane_stride", depth_plane_stride=v)
    for v in (-1, 7):
        refused(f, ARG, "bits_plane_stride", bits_plane_stride=v)
        refused(f, ARG, "out_plane_stride", out_plane_stride=v)
    refused(f, ARG, "bits_plane_stride", H=9, W=33, depth_plane_stride=297, bits_plane_stride=9, out_plane_stride=10)     # 297 bits: 10 words
    refused(f, ARG, "nothing to do", out_bits=None, counts=None, levels=None)
    refused(f, ARG, "NULL", depth=None)
    refused(f, ARG, "NULL", mask_bits=None)
    for name, base in (("depth", 16384), ("mask_bits", 0), ("out_bits", 4096), ("counts", 8192), ("levels", 12288), ("image_index", 20480)):
        for d in (1, 2, 3):
            refused(f, ARG, "4-byte aligned", **{name: f.p + base + d})
    # the rank: the first rule that fails speaks
    refused(f, ARG, "struct_size", size=8, B=-1)
    refused(f, ARG, "B >= 0", B=-1, frame_width=40)
    refused(f, ARG, "frame_width", frame_width=40, k=-1.0)
    refused(f, ARG, "k must be", k=-1.0, min_band=-1.0)
    refused(f, ARG, "min_band must be", min_band=-1.0, near=NAN)
    refused(f, ARG, "near and far", near=NAN, bits_plane_stride=7)
    refused(f, ARG, "bits_plane_stride", bits_plane_stride=7, H=2048, W=1024, depth_plane_stride=0)
    refused(f, UNSUPPORTED, "857728", H=2048, W=1024, depth_plane_stride=0, bits_plane_stride=0, out_plane_stride=0, mask_bits=None)
    # the rules hold for an empty batch too; a valid empty batch is success without a launch, whatever the pointers
    refused(f, ARG, "k must be", B=0, k=NAN)
    refused(f, UNSUPPORTED, "857728", B=0, H=2048, W=1024, depth_plane_stride=0, bits_plane_stride=0, out_plane_stride=0)
    assert call(f, B=0)[0] == 0
    assert call(f, B=0, depth=None, mask_bits=None, out_bits=None, counts=None, levels=None)[0] == 0
    assert call(f, B=0, mask_bits=f.p + 1, out_bits=f.p)[0] == 0
    # what is allowed gets past every rule: +-inf for near / far, zero strides, statistics only, in place - each refused only by the
    # rule placed behind them (a misaligned levels pointer)
    for kw in (dict(near=-INF, far=INF), dict(near=INF, far=-INF), dict(depth_plane_stride=0, bits_plane_stride=0, out_plane_stride=0),
               dict(out_bits=None), dict(out_bits=f.p), dict(frame_width=32), dict(frame_width=1), dict(k=0.0, min_band=0.0)):
        refused(f, ARG, "4-byte aligned", levels=f.p + 12289, **kw)


def test_c_entry_refuses_partial_overlap_and_takes_in_place():
    f = Fake()
    bad = f.p + 12289          # (a misaligned levels pointer: the rule behind the overlap rule)
    refused(f, ARG, "overlap", out_bits=f.p + 4 * 15)                       # the last word of the input range
    refused(f, ARG, "overlap", mask_bits=f.p + 4096 + 4 * 15)               # the input begins inside the output range
    refused(f, ARG, "overlap", out_bits=f.p + 4)                            # shifted by a word
    refused(f, ARG, "overlap", out_bits=f.p, out_plane_stride=9)            # the same base, other strides
    refused(f, ARG, "overlap", bits_plane_stride=600, out_bits=f.p + 2048)  # long strides: planes of one lie between planes of the other
    refused(f, ARG, "overlap", bits_plane_stride=0, out_plane_stride=0, out_bits=f.p + 4 * 15)   # stride 0 = the words of a plane
    refused(f, ARG, "4-byte aligned", out_bits=f.p, levels=bad)             # exactly in place: not an overlap
    refused(f, ARG, "4-byte aligned", out_bits=f.p, bits_plane_stride=0, out_plane_stride=8, levels=bad)   # 0 = 8 words: equal strides
    refused(f, ARG, "4-byte aligned", out_bits=f.p, bits_plane_stride=24, out_plane_stride=24, levels=bad)


def test_c_entry_unsupported_sizes():
    f = Fake()
    free = dict(depth_plane_stride=0, bits_plane_stride=0, out_plane_stride=0)
    refused(f, UNSUPPORTED, "857728", H=857729, W=1, **free)
    refused(f, UNSUPPORTED, "857728", H=1024, W=1024, **free)
    refused(f, UNSUPPORTED, "857728", H=1 << 20, W=1 << 20, **free)          # no 32-bit wrap
    # the documented bound itself, and the 819200 pixels the ratio median takes, pass the size rule (the next rule speaks)
    refused(f, ARG, "NULL", H=857728, W=1, mask_bits=None, **free)
    refused(f, ARG, "NULL", H=640, W=1280, mask_bits=None, **free)
    refused(f, ARG, "NULL", H=480, W=640, mask_bits=None, **free)


def test_python_argument_errors_come_before_any_device_work():
    import torch

    import labelany3d_amd as la

    mb = la.MaskBits(torch.zeros((2, 8), dtype=torch.int32), 8, 32, 32)     # on the host: never reaches a device
    depth = torch.zeros((8, 32), dtype=torch.float32)
    for fn in (la.gate_depth_bits, la.depth_gate_stats):
        for v in (-1, -0.5, NAN, INF, 1e39, True, "3", None):
            with pytest.raises(ValueError, match="k must be"):
                fn(depth, mb, k=v)
            with pytest.raises(ValueError, match="min_band must be"):
                fn(depth, mb, min_band=v)
        for v in (NAN, True, "3", np.float32("nan")):
            with pytest.raises(ValueError, match="near must be"):
                fn(depth, mb, near=v)
            with pytest.raises(ValueError, match="far must be"):
                fn(depth, mb, far=v)
        with pytest.raises(ValueError, match="must be a MaskBits"):
            fn(depth, (mb.bits, 8, 32, 32))
        with pytest.raises(ValueError, match="must be a MaskBits"):
            fn(depth, mb.bits)
        with pytest.raises(ValueError, match="Depth16"):
            fn(la.Depth16(torch.zeros((8, 32), dtype=torch.float16)), mb)
        for dt in (torch.float16, torch.float64, torch.int32, torch.uint16):
            with pytest.raises(ValueError, match="must be float32"):
                fn(torch.zeros((8, 32), dtype=dt), mb)
        with pytest.raises(ValueError, match="must be float32"):
            fn(np.zeros((8, 32), np.float64), mb)
        with pytest.raises(ValueError, match="on the GPU"):
            fn(depth, mb)
        with pytest.raises(ValueError, match="frame_width"):
            fn(depth, la.MaskBits(mb.bits, 8, 32, 33))
    with pytest.raises(TypeError):
        la.depth_gate_stats(depth, mb, out=mb.bits)                          # the statistics-only call has no planes to place
