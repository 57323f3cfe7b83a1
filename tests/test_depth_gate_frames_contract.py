"""CPU-only tests of the frames form of the depth gate on bit planes (include/la3d.h "depth gate on bit planes",
la3d_depth_gate_bits_frames; ``gate_depth_bits_frames``, ``depth_gate_stats_frames``): the case lists, the names on every layer, the
layout of the argument block, the C entry's refusals before any launch in their stated order (fake pointers: nothing here reaches a
device) and the Python argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import depth16_cases as D16
from . import depth_gate_cases as DG
from . import depth_gate_frames_cases as XG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2
INF, NAN = float("inf"), float("nan")
WHO = b"la3d_depth_gate_bits_frames: "


def test_the_case_lists_are_what_they_say():
    assert len(XG.SIZES) == 12 and XG.B == 24 and (1, 1) in XG.SIZES and (140, 96) in XG.SIZES
    assert {XG.depth_kind(p) for p in range(12)} == set(XG.DEPTH_KINDS) and {XG.mask_kind(b) for b in range(24)} == set(XG.MASK_KINDS)
    for m, p, d in zip(XG.masks(), XG.IMAGE_INDEX, [XG.depth_maps()[p] for p in XG.IMAGE_INDEX]):
        assert m.shape == d.shape == XG.SIZES[p] and d.dtype == np.float32
    # the scalars are not idle on the list: every set changes some row against the defaults, or is the defaults
    base = XG.expected(0)
    assert (base[1][:, 2] < base[1][:, 1]).any() and (base[1][:, 1] < base[1][:, 0]).any() and (base[1][:, 1] == 0).any()
    for i in range(1, len(DG.PARAMS)):
        assert (XG.expected(i)[1] != base[1]).any() or not np.array_equal(XG.expected(i)[2], base[2], equal_nan=True), DG.PARAMS[i]
    # 16-bit: stored zeros lie under masks in both flag states, and the flag decides whether they are valid
    for variant in D16.VARIANTS:
        dtype, scale, hole = variant
        st = XG.stored(variant)
        assert all(s.dtype == (np.float16 if dtype == "f16" else np.uint16) for s in st)
        if dtype == "u16":
            zeros = [int((st[p] == 0)[m].sum()) for m, p in zip(XG.masks(), XG.IMAGE_INDEX)]
            assert sum(z > 0 for z in zeros) >= 4, variant
            cnt = XG.expected(0, variant)[1]
            with_zero = [b for b, z in enumerate(zeros) if z > 0]
            if hole:
                assert all(cnt[b, 1] <= cnt[b, 0] - zeros[b] for b in with_zero)
            else:
                assert any(cnt[b, 1] == cnt[b, 0] for b in with_zero)
            # a row whose median falls between two quantisation steps: an even count whose two middle stored words differ
            between = 0
            for b, (m, p) in enumerate(zip(XG.masks(), XG.IMAGE_INDEX)):
                up = XG.upconverted(variant)[p]
                v = np.sort(up[m & np.isfinite(up)])
                if v.size and v.size % 2 == 0 and v[v.size // 2 - 1] != v[v.size // 2]:
                    med = XG.expected(0, variant)[2][b, 0]
                    between += int(v[v.size // 2 - 1] < med < v[v.size // 2])
            assert between >= 2, variant
    # the second list: counts on both sides of the 6144 keys of the fast path, small images in front, between and behind
    sizes, depths, row_masks, ii = XG.big_list()
    nv = XG.big_expected(0)[1][:, 1]
    assert (nv > 6144).sum() >= 6 and ((nv > 512) & (nv <= 6144)).sum() >= 2 and (nv < 64).sum() >= 2
    assert sizes[0] == XG.SMALL[0] and sizes[-1] == XG.SMALL[2] and sizes.count(DG.BIG) == len(DG.big_planes()[0]) and len(sizes) == len(depths)
    assert max(h for h, _ in sizes) == 96 and max((w + 31) // 32 * 32 for _, w in sizes) == 96 and XG.BIG_BOUNDS[0] > 96 < XG.BIG_BOUNDS[1]
    assert (np.diff(ii) >= 0).all() and len(ii) == len(row_masks)


def test_names_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _lib, bits, frames, masks, morph

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    assert re.search(r"\bint la3d_depth_gate_bits_frames\s*\(\s*const la3d_depth_gate_frames_args\s*\*", hdr)
    assert "typedef struct la3d_depth_gate_frames_args" in hdr and "-2, 0, 0" in hdr
    assert "la3d_depth_gate_bits_frames" in _lib.EXPORTS and hasattr(_lib.lib, "la3d_depth_gate_bits_frames")
    assert issubclass(_lib.DepthGateFramesArgs, C.Structure)
    for fn in ("gate_depth_bits_frames", "depth_gate_stats_frames"):
        assert callable(getattr(la, fn)) and fn in la.__all__ and getattr(morph, fn) is getattr(la, fn) is getattr(masks, fn), fn
    assert not re.search(r"^\s*(from|import)\b.*\bmorph\b", open(frames.__file__).read(), re.M)      # frames.py and bits.py stand below
    assert not re.search(r"^\s*(from|import)\b.*\bmorph\b", open(bits.__file__).read(), re.M)
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2     # additive
    assert C.sizeof(_lib.DepthGateArgs) == 120                                                  # the uniform block is untouched
    assert "in place" in la.gate_depth_bits_frames.__doc__ and "PackedFrames16" in la.gate_depth_bits_frames.__doc__


def test_block_layout_matches_the_header():
    """the ctypes block against the header's text: the same fields in the same order with the same types, the natural offsets, and
    the size the header states"""
    from labelany3d_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    stated, body = re.search(r"typedef struct la3d_depth_gate_frames_args \{\s*/\* (\d+) bytes \*/(.*?)\} la3d_depth_gate_frames_args;", hdr, re.S).groups()
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
    got = list(_lib.DepthGateFramesArgs._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, t), (_, w) in zip(got, want):
        assert C.sizeof(t) == C.sizeof(w) and C.alignment(t) == C.alignment(w), n
    off = 0
    for n, t in want:
        off = (off + C.alignment(t) - 1) // C.alignment(t) * C.alignment(t)
        assert getattr(_lib.DepthGateFramesArgs, n).offset == off, n
        off += C.sizeof(t)
    assert C.sizeof(_lib.DepthGateFramesArgs) == int(stated) == 152 == (off + 7) // 8 * 8
    A = _lib.DepthGateFramesArgs
    assert (A.P.offset, A.k.offset, A.reserved.offset, A.depth.offset, A.depth16.offset, A.depth_elems.offset, A.frames.offset, A.bits.offset,
            A.out_bits.offset, A.counts.offset, A.stream.offset) == (8, 20, 36, 40, 48, 56, 64, 80, 104, 128, 144)


class Fake:
    """fake "device" memory, 64-byte aligned: every call below is refused, or has nothing to do, before any launch"""

    def __init__(self):
        self.buf = (C.c_char * 32768)()
        self.p = (C.addressof(self.buf) + 63) & ~63


BASE = dict(bits=0, bits_offsets=2048, frames=4096, image_index=6144, out_bits=8192, out_offsets=10240, counts=12288, levels=14336, depth=16384)


def d16(f, **kw):
    from labelany3d_amd import _lib

    a = dict(struct_size=C.sizeof(_lib.Depth16Block), dtype=_lib.DTYPE_U16, planes=f.p + BASE["depth"], plane_stride=0, scale=0.001,
             flags=_lib.DEPTH_ZERO_IS_HOLE)
    a.update(kw)
    return C.pointer(_lib.Depth16Block(**a))


def call(f, size=None, **kw):
    from labelany3d_amd import _lib

    a = dict(B=2, P=2, H=8, W=32, k=4.5, min_band=0.0, near=-INF, far=INF, reserved=0, depth=f.p + BASE["depth"], depth16=None, depth_elems=512,
             frames=f.p + BASE["frames"], image_index=f.p + BASE["image_index"], bits=f.p, bits_words=64, bits_offsets=f.p + BASE["bits_offsets"],
             out_bits=f.p + BASE["out_bits"], out_words=64, out_offsets=f.p + BASE["out_offsets"], counts=f.p + BASE["counts"],
             levels=f.p + BASE["levels"], stream=None)
    a.update(kw)
    blk = _lib.DepthGateFramesArgs(struct_size=C.sizeof(_lib.DepthGateFramesArgs) if size is None else size, **a)
    rc = _lib.lib.la3d_depth_gate_bits_frames(C.byref(blk))
    return rc, _lib.lib.la3d_last_error()


def refused(f, code, word, **kw):
    rc, msg = call(f, **kw)
    assert rc == code and word.encode() in msg and msg.startswith(WHO), (kw, rc, msg)


def test_c_entry_refuses_before_any_launch():
    from labelany3d_amd import _lib

    f = Fake()
    for size in (0, 120, 144, 151, 153, 160, -1):
        refused(f, ARG, "struct_size", size=size)
    assert _lib.lib.la3d_depth_gate_bits_frames(None) == ARG and _lib.lib.la3d_last_error().startswith(WHO)
    for kw in (dict(B=-1), dict(P=-1), dict(H=0), dict(W=0), dict(H=-3), dict(W=-1)):
        refused(f, ARG, "B, P >= 0, bounds H, W > 0", **kw)
    for v in (-1.0, -1e-30, NAN, INF, -INF):
        refused(f, ARG, "k must be", k=v)
        refused(f, ARG, "min_band must be", min_band=v)
    refused(f, ARG, "near and far", near=NAN)
    refused(f, ARG, "near and far", far=NAN)
    for v in (1, -1, 255):
        refused(f, ARG, "reserved", reserved=v)
    refused(f, ARG, "exactly one of depth / depth16", depth=None)
    refused(f, ARG, "exactly one of depth / depth16", depth16=d16(f))
    for bad in (dict(struct_size=16), dict(struct_size=0)):
        refused(f, ARG, "struct_size of la3d_depth16", depth=None, depth16=d16(f, **bad))
    for dt in (_lib.DTYPE_F32, _lib.DTYPE_BF16, 7, -1):
        refused(f, ARG, "unknown dtype", depth=None, depth16=d16(f, dtype=dt))
    for sc in (0.0, -0.001, NAN, INF):
        refused(f, ARG, "finite scale > 0", depth=None, depth16=d16(f, scale=sc))
    refused(f, ARG, "flags", depth=None, depth16=d16(f, flags=2))
    refused(f, ARG, "flags", depth=None, depth16=d16(f, dtype=_lib.DTYPE_F16, flags=1))
    for v in (1, 256, -4):
        refused(f, ARG, "plane_stride must be 0", depth=None, depth16=d16(f, plane_stride=v))
    refused(f, ARG, "planes is NULL", depth=None, depth16=d16(f, planes=None))
    refused(f, ARG, "must not be negative", depth_elems=-1)
    refused(f, ARG, "must not be negative", bits_words=-1)
    refused(f, ARG, "must not be negative", out_words=-1)
    assert call(f, out_words=-1, out_bits=None, out_offsets=None, B=0)[0] == 0        # out_words is not read without out_bits
    for name in ("bits", "out_bits"):
        for d in (4, 8, 12):
            refused(f, ARG, "16-byte aligned", **{name: f.p + BASE[name] + d})
    for d in (4, 8, 12):
        refused(f, ARG, "depth buffer must be 16-byte", depth=f.p + BASE["depth"] + d)
    for d in (2, 4, 6):
        refused(f, ARG, "depth buffer must be 16-byte", depth=None, depth16=d16(f, planes=f.p + BASE["depth"] + d))
    assert call(f, depth=None, depth16=d16(f, planes=f.p + BASE["depth"] + 8), B=0)[0] == 0        # 8 bytes serve 16-bit planes
    for name in ("bits_offsets", "out_offsets", "frames"):
        refused(f, ARG, "8-byte aligned", **{name: f.p + BASE[name] + 4})
    for name in ("image_index", "counts", "levels"):
        for d in (1, 2, 3):
            refused(f, ARG, "4-byte aligned", **{name: f.p + BASE[name] + d})
    refused(f, ARG, "nothing to do", out_bits=None, counts=None, levels=None)
    for name in ("bits", "bits_offsets", "image_index", "frames"):
        refused(f, ARG, "NULL", **{name: None})
    refused(f, ARG, "out_offsets must not be NULL", out_offsets=None)
    assert call(f, P=0, frames=None, B=0)[0] == 0
    # what is allowed gets past every argument rule: each is refused only by a rule placed behind (NULL image_index with B > 0)
    for kw in (dict(near=-INF, far=INF), dict(near=INF, far=-INF), dict(out_bits=None, out_offsets=None), dict(k=0.0, min_band=0.0),
               dict(counts=None), dict(levels=None), dict(depth=None, depth16=d16(f)), dict(depth=None, depth16=d16(f, dtype=_lib.DTYPE_F16, flags=0)),
               dict(depth=None, depth16=d16(f, flags=0)), dict(depth_elems=0), dict(P=0, frames=None)):
        refused(f, ARG, "NULL bits, bits_offsets, image_index or frames", image_index=None, **kw)


def test_c_entry_refusals_come_in_the_stated_order():
    """the first rule that fails speaks: each rule set against the one after it"""
    from labelany3d_amd import _lib

    f = Fake()
    p = f.p
    refused(f, ARG, "struct_size", size=8, B=-1)
    refused(f, ARG, "B, P >= 0", P=-1, k=-1.0)
    refused(f, ARG, "k must be", k=-1.0, min_band=-1.0)
    refused(f, ARG, "min_band must be", min_band=-1.0, near=NAN)
    refused(f, ARG, "near and far", near=NAN, reserved=1)
    refused(f, ARG, "reserved", reserved=1, depth=None)
    refused(f, ARG, "exactly one", depth16=d16(f, dtype=9), depth_elems=-1)
    refused(f, ARG, "unknown dtype", depth=None, depth16=d16(f, dtype=9, scale=0.0), depth_elems=-1)
    refused(f, ARG, "finite scale", depth=None, depth16=d16(f, scale=0.0, plane_stride=8), depth_elems=-1)
    refused(f, ARG, "plane_stride", depth=None, depth16=d16(f, plane_stride=8), depth_elems=-1)
    refused(f, ARG, "must not be negative", depth_elems=-1, bits=p + 4)
    refused(f, ARG, "16-byte aligned", bits=p + 4, depth=p + BASE["depth"] + 8)
    refused(f, ARG, "depth buffer", depth=p + BASE["depth"] + 8, frames=p + BASE["frames"] + 4)
    refused(f, ARG, "8-byte aligned", frames=p + BASE["frames"] + 4, counts=p + BASE["counts"] + 2)
    refused(f, ARG, "4-byte aligned", image_index=p + BASE["image_index"] + 2, out_bits=None, counts=None, levels=None)
    refused(f, ARG, "nothing to do", out_bits=None, counts=None, levels=None, bits=None)
    refused(f, ARG, "overlap", out_bits=p + 16, image_index=None)
    refused(f, ARG, "NULL", image_index=None, H=2048, W=1024)
    refused(f, ARG, "out_offsets must not be NULL", out_offsets=None, H=2048, W=1024)
    refused(f, UNSUPPORTED, "857728", H=2048, W=1024)
    # the rules hold for an empty batch too; a valid empty batch is success without a launch, whatever the input pointers
    refused(f, ARG, "k must be", B=0, k=NAN)
    refused(f, ARG, "reserved", B=0, reserved=3)
    refused(f, ARG, "exactly one", B=0, depth=None)
    refused(f, ARG, "finite scale", B=0, depth=None, depth16=d16(f, scale=-1.0))
    refused(f, ARG, "16-byte aligned", B=0, out_bits=p + BASE["out_bits"] + 8)
    refused(f, ARG, "nothing to do", B=0, out_bits=None, counts=None, levels=None)
    refused(f, ARG, "overlap", B=0, out_bits=p + 16)
    refused(f, UNSUPPORTED, "857728", B=0, H=2048, W=1024)
    assert call(f, B=0)[0] == 0 and call(f, B=0, P=0)[0] == 0
    assert call(f, B=0, bits=None, bits_offsets=None, frames=None, image_index=None, out_offsets=None)[0] == 0
    assert _lib.lib.la3d_last_error().startswith(WHO)                      # (of the last refusal: success does not clear it)


def test_c_entry_takes_in_place_and_refuses_every_other_overlap():
    f = Fake()
    offs = f.p + BASE["bits_offsets"]
    same = dict(out_bits=f.p, out_words=64, out_offsets=offs)
    refused(f, ARG, "NULL", image_index=None, **same)                      # exactly in place: past the overlap rule
    refused(f, ARG, "overlap", **dict(same, out_words=63))                 # the same base, another length
    refused(f, ARG, "overlap", **dict(same, out_offsets=f.p + BASE["out_offsets"]))   # the same buffer, other offsets
    refused(f, ARG, "overlap", out_bits=f.p + 4 * 60)                      # the last words of the input range
    refused(f, ARG, "overlap", bits=f.p + BASE["out_bits"] + 4 * 60)       # the input begins inside the output range
    refused(f, ARG, "overlap", bits_words=4096, out_bits=f.p + BASE["out_bits"])      # a long input buffer that holds the output
    refused(f, ARG, "overlap", out_bits=f.p + 16)
    assert call(f, out_bits=f.p + 256, B=0)[0] == 0                        # side by side: [p, p + 256) and [p + 256, p + 512)


def test_c_entry_unsupported_bounds_at_the_edge_and_one_beyond():
    f = Fake()
    refused(f, UNSUPPORTED, "857728", H=1024, W=1024)
    refused(f, UNSUPPORTED, "857728", H=26805, W=32)                       # 26805 * 32 = 857760
    refused(f, UNSUPPORTED, "857728", H=26804, W=33)                       # roundup32(33) = 64
    refused(f, UNSUPPORTED, "857728", H=(1 << 31) - 1, W=(1 << 31) - 1)    # no 32-bit wrap
    # the documented bound itself passes the size rule: a valid empty batch, and with B > 0 the next rule speaks
    assert call(f, B=0, H=26804, W=32)[0] == 0 and call(f, B=0, H=640, W=1280)[0] == 0 and call(f, B=0, H=640, W=640)[0] == 0
    assert call(f, B=0, H=26804, W=1)[0] == 0                              # one column is stored 32 wide
    refused(f, ARG, "NULL", H=26804, W=32, bits=None)


def host_frames(sizes, dtype=None):
    import labelany3d_amd as la

    maps = [np.zeros(s, np.float32 if dtype is None else np.float16 if dtype == "f16" else np.uint16) for s in sizes]
    return la.pack_frames(maps, device="cpu", dtype=dtype)


def host_bits(frames, ii):
    import torch

    import labelany3d_amd as la

    offs, total = la.frame_bits_offsets(frames.table_host, ii)
    return la.FrameBits(torch.zeros(max(total, 4), dtype=torch.int32), torch.as_tensor(offs), torch.as_tensor(np.asarray(ii, np.int32)),
                        torch.zeros(len(ii), dtype=torch.int32), frames.table_host, frames.H, frames.W)


def test_python_argument_errors_come_before_any_device_work(monkeypatch):
    import torch

    import labelany3d_amd as la
    from labelany3d_amd import morph

    class Reached:
        """stands in for the library: reaching the C entry fails the test"""

        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    monkeypatch.setattr(morph, "lib", Reached())
    pf = host_frames(XG.SIZES)                                             # on the host: never reaches a device
    fb = host_bits(pf, XG.IMAGE_INDEX)
    every = (la.gate_depth_bits_frames, la.depth_gate_stats_frames)
    # 1  a frames that carries no depth: the other kinds an entry that reads only the table takes, and what is no frames at all
    grid = la.FrameGrid(pf.table, pf.table_host, pf.H, pf.W, list(pf.sizes))
    labels = la.pack_label_frames([np.zeros(s, np.uint8) for s in XG.SIZES], device="cpu")
    stacks = la.pack_mask_frames([np.zeros((1,) + s, np.uint8) for s in XG.SIZES], device="cpu")
    for fn in every:
        for fr in (grid, labels, stacks, pf.table_host, pf.depth, None):
            with pytest.raises(ValueError, match="frames must be the PackedFrames / PackedFrames16"):
                fn(fr, fb)
        with pytest.raises(ValueError, match="Depth16"):
            fn(la.Depth16(torch.zeros((8, 32), dtype=torch.float16)), fb)
    # 2  a foreign table, or no FrameBits at all
    other = host_frames(XG.SIZES[:-1] + ((32, 161),))
    for fn in every:
        with pytest.raises(ValueError, match="another frame table"):
            fn(other, fb)
        with pytest.raises(ValueError, match="must be the FrameBits"):
            fn(pf, (fb.bits, fb.offsets))
        with pytest.raises(ValueError, match="must be the FrameBits"):
            fn(pf, la.MaskBits(fb.bits.view(1, -1), 8, 32, 32))
    # 3  the scalars, with the messages of the uniform functions
    for fn in every:
        for v in (-1, -0.5, NAN, INF, 1e39, True, "3", None):
            with pytest.raises(ValueError, match="k must be"):
                fn(pf, fb, k=v)
            with pytest.raises(ValueError, match="min_band must be"):
                fn(pf, fb, min_band=v)
        for v in (NAN, True, "3", np.float32("nan")):
            with pytest.raises(ValueError, match="near must be"):
                fn(pf, fb, near=v)
            with pytest.raises(ValueError, match="far must be"):
                fn(pf, fb, far=v)
    # 4  bounds beyond the LDS limit
    big = host_frames([(1024, 1024)])
    for fn in every:
        with pytest.raises(ValueError, match="857728 stored pixels"):
            fn(big, host_bits(big, [0]))
    # 5  a bad out: not flat, another dtype, too short, on the host, strided, no tensor; overlapping without being the input
    n = fb.bits.numel()
    for out in (torch.zeros((2, n), dtype=torch.int32), torch.zeros(n, dtype=torch.int64), torch.zeros(n - 1, dtype=torch.int32),
                torch.zeros(n, dtype=torch.int32), torch.zeros(2 * n, dtype=torch.int32)[::2], np.zeros(n, np.int32), "out"):
        with pytest.raises(ValueError, match="out must be"):
            la.gate_depth_bits_frames(pf, fb, out=out)
    for out in (fb.bits[4:], fb.bits[:8], fb.bits[:-4]):
        with pytest.raises(ValueError, match="overlaps"):
            la.gate_depth_bits_frames(pf, fb, out=out)
    with pytest.raises(TypeError):
        la.depth_gate_stats_frames(pf, fb, out=fb.bits)                     # the statistics-only call has no planes to place
    # the last check of all: where the buffers live (16-bit frames and the in-place form get this far too)
    for fr in (pf, host_frames(XG.SIZES, "f16"), host_frames(XG.SIZES, "u16")):
        for fn in every:
            with pytest.raises(ValueError, match="on the GPU"):
                fn(fr, fb)
        with pytest.raises(ValueError, match="on the GPU"):
            la.gate_depth_bits_frames(fr, fb, out=fb.bits)
