"""CPU-only tests of the frames form of connected components on bit planes (include/la3d.h "connected components on bit planes",
la3d_components_bits_frames): the names on every layer, the layout of the argument block, the C entry's refusals before any launch
in their stated order (fake pointers: nothing here reaches a device), the Python argument errors, and the NumPy restatement against
SciPy on the mixed-size case list."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import components_cases as CC
from . import components_frames_cases as XC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2
WHO = b"la3d_components_bits_frames: "


def test_the_case_list_is_what_it_says():
    named = XC.cases()
    assert len(XC.SIZES) == 12 and len(named) == len(XC.IMAGE_INDEX) == 24 and len({n for n, _ in named}) == 24
    for (name, m), p in zip(named, XC.IMAGE_INDEX):
        assert m.shape == XC.SIZES[p] and CC.count_runs(m) <= CC.MAX_CASE_RUNS, name
    kinds = {n.split("_")[0] for n, _ in named}
    assert {"spiral", "comb", "checkerboard", "diagonals", "ring", "seams", "equal", "area", "empty", "full", "blob"} == kinds
    assert (1, 1) in XC.SIZES and (140, 96) in XC.SIZES and sum(w % 32 != 0 for _, w in XC.SIZES) >= 6
    # the rules are not idle on the list: some planes change under each rule, and the two connectivities differ
    for min_area, largest in XC.RULES4[1:]:
        outs, stats, _ = XC.expected(8, min_area, largest)
        assert sum(not np.array_equal(o, m) for o, (_, m) in zip(outs, named)) >= 6, (min_area, largest)
    assert (XC.expected(4, 0, False)[1][:, 0] != XC.expected(8, 0, False)[1][:, 0]).sum() >= 6
    assert (XC.expected(8, 0, False)[1][:, 0] > XC.TABLE_ROWS).any() and (XC.expected(8, 0, False)[1][:, 0] < XC.TABLE_ROWS).any()


def test_restatement_equals_scipy_on_every_mixed_size_case():
    ndi = pytest.importorskip("scipy.ndimage")
    structure = {4: ndi.generate_binary_structure(2, 1), 8: np.ones((3, 3), int)}
    for name, m in XC.cases():
        for conn in XC.CONNECTIVITIES:
            want, n = ndi.label(m, structure[conn])
            got, k, _ = XC.labelled(name, m, conn)
            assert k == n and np.array_equal(got, want), (name, conn)


def test_names_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _lib, components, frames

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    assert re.search(r"\bint la3d_components_bits_frames\s*\(\s*const la3d_components_frames_args\s*\*", hdr)
    assert "typedef struct la3d_components_frames_args" in hdr and "-2, 0, 0, 0, 0, 0, 0, 0" in hdr
    assert "la3d_components_bits_frames" in _lib.EXPORTS and hasattr(_lib.lib, "la3d_components_bits_frames")
    assert issubclass(_lib.ComponentsFramesArgs, C.Structure)
    for fn in ("components_bits_frames", "components_stats_frames", "largest_component_bits_frames", "drop_islands_bits_frames"):
        assert callable(getattr(la, fn)) and fn in la.__all__ and getattr(components, fn) is getattr(la, fn), fn
    assert not re.search(r"^\s*(from|import)\b.*\bcomponents\b", open(frames.__file__).read(), re.M)      # frames.py does not import components
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2     # additive
    assert C.sizeof(_lib.ComponentsArgs) == 104                                                 # the uniform block is untouched


def test_block_layout_matches_the_header():
    """the ctypes block against the header's text: the same fields in the same order with the same types, and the natural offsets"""
    from labelany3d_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    body = re.search(r"typedef struct la3d_components_frames_args \{(.*?)\} la3d_components_frames_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        base, star, names = m.group(1), m.group(2), m.group(3)
        for nm in names.split(","):
            arr = re.match(r"(\w+)\s*\[(\d+)\]", nm.strip())
            if arr:
                want.append((arr.group(1), ctype[base] * int(arr.group(2))))
            else:
                want.append((nm.strip(), C.c_void_p if star else ctype[base]))
    got = [(n, t) for n, t in _lib.ComponentsFramesArgs._fields_]
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, t), (_, w) in zip(got, want):
        assert C.sizeof(t) == C.sizeof(w) and C.alignment(t) == C.alignment(w) and (t is w or getattr(t, "_length_", 0) == getattr(w, "_length_", -1)), n
    off = 0
    for n, t in want:
        off = (off + C.alignment(t) - 1) // C.alignment(t) * C.alignment(t)
        assert getattr(_lib.ComponentsFramesArgs, n).offset == off, n
        off += C.sizeof(t)
    assert C.sizeof(_lib.ComponentsFramesArgs) == 144 == (off + 7) // 8 * 8
    A = _lib.ComponentsFramesArgs
    assert (A.P.offset, A.H.offset, A.reserved.offset, A.bits.offset, A.frames.offset, A.out_bits.offset, A.stats.offset, A.stream.offset) == \
        (8, 12, 40, 48, 72, 88, 112, 136)


class Fake:
    """fake "device" memory, 64-byte aligned: every call below is refused, or has nothing to do, before any launch"""

    def __init__(self):
        self.buf = (C.c_char * 32768)()
        self.p = (C.addressof(self.buf) + 63) & ~63


def call(f, size=None, reserved=(0, 0), **kw):
    from labelany3d_amd import _lib

    a = dict(B=2, P=2, H=8, W=32, connectivity=8, min_area=0, largest=0, max_runs=64, max_components=4,
             bits=f.p, bits_words=64, bits_offsets=f.p + 2048, frames=f.p + 4096, image_index=f.p + 6144,
             out_bits=f.p + 8192, out_words=64, out_offsets=f.p + 10240, stats=f.p + 12288, components=f.p + 14336,
             workspace=f.p + 16384, stream=None)
    a.update(kw)
    blk = _lib.ComponentsFramesArgs(struct_size=C.sizeof(_lib.ComponentsFramesArgs) if size is None else size, **a)
    blk.reserved[0], blk.reserved[1] = reserved
    rc = _lib.lib.la3d_components_bits_frames(C.byref(blk))
    return rc, _lib.lib.la3d_last_error()


def refused(f, code, word, **kw):
    rc, msg = call(f, **kw)
    assert rc == code and word.encode() in msg and msg.startswith(WHO), (kw, rc, msg)


BASE = dict(bits=0, bits_offsets=2048, frames=4096, image_index=6144, out_bits=8192, out_offsets=10240, stats=12288, components=14336,
            workspace=16384)


def test_c_entry_refuses_before_any_launch():
    from labelany3d_amd import _lib

    f = Fake()
    for size in (0, 104, 136, 143, 145, 152, -1):
        refused(f, ARG, "struct_size", size=size)
    assert _lib.lib.la3d_components_bits_frames(None) == ARG
    for kw in (dict(B=-1), dict(P=-1), dict(H=0), dict(W=0), dict(H=-3), dict(W=-1)):
        refused(f, ARG, "B, P >= 0, bounds H, W > 0", **kw)
    for c in (0, 1, 6, 9, -8, 26):
        refused(f, ARG, "connectivity", connectivity=c)
    for v in (2, -1, 255):
        refused(f, ARG, "largest", largest=v)
    refused(f, ARG, "min_area", min_area=-1)
    for v in (0, -1, -(1 << 31)):
        refused(f, ARG, "max_runs", max_runs=v)
    refused(f, ARG, "max_components", max_components=-1)
    refused(f, ARG, "max_components > 0", max_components=0)                 # components without rows
    refused(f, ARG, "nothing to do", out_bits=None, stats=None, components=None)
    for r in ((1, 0), (0, 1), (-1, -1)):
        refused(f, ARG, "reserved", reserved=r)
    refused(f, ARG, "must not be negative", bits_words=-1)
    refused(f, ARG, "must not be negative", out_words=-1)
    assert call(f, out_words=-1, out_bits=None, out_offsets=None, B=0)[0] == 0        # out_words is not read without out_bits
    for name in ("bits", "out_bits"):
        for d in (4, 8, 12):
            refused(f, ARG, "16-byte aligned", **{name: f.p + BASE[name] + d})
    for name in ("bits_offsets", "out_offsets", "frames"):
        refused(f, ARG, "8-byte aligned", **{name: f.p + BASE[name] + 4})
    for name in ("stats", "components", "workspace", "image_index"):
        for d in (1, 2, 3):
            refused(f, ARG, "4-byte aligned", **{name: f.p + BASE[name] + d})
    for name in ("bits", "bits_offsets", "image_index", "workspace", "frames"):
        refused(f, ARG, "NULL", **{name: None})
    refused(f, ARG, "out_offsets must not be NULL", out_offsets=None)
    assert call(f, P=0, frames=None, B=0)[0] == 0


def test_c_entry_refusals_come_in_the_stated_order():
    """the first rule that fails speaks: each rule set against the one after it"""
    f = Fake()
    p = f.p
    refused(f, ARG, "struct_size", size=8, B=-1)
    refused(f, ARG, "B, P >= 0", P=-1, connectivity=5)
    refused(f, ARG, "connectivity", connectivity=5, largest=2)
    refused(f, ARG, "largest", largest=2, min_area=-1)
    refused(f, ARG, "min_area", min_area=-1, max_runs=0)
    refused(f, ARG, "max_runs", max_runs=0, max_components=-1)
    refused(f, ARG, "max_components must not", max_components=-1, out_bits=None, stats=None, components=None)
    refused(f, ARG, "max_components > 0", max_components=0, reserved=(1, 0))
    refused(f, ARG, "nothing to do", out_bits=None, stats=None, components=None, reserved=(1, 0))
    refused(f, ARG, "reserved", reserved=(0, 7), bits_words=-1)
    refused(f, ARG, "must not be negative", bits_words=-1, bits=p + 4)
    refused(f, ARG, "16-byte aligned", bits=p + 4, frames=p + 4096 + 4)
    refused(f, ARG, "8-byte aligned", frames=p + 4096 + 4, stats=p + 12288 + 2)
    refused(f, ARG, "4-byte aligned", stats=p + 12288 + 2, out_bits=p)
    refused(f, ARG, "overlap", out_bits=p, image_index=None)
    refused(f, ARG, "NULL", image_index=None, H=2048, W=1024)
    refused(f, ARG, "out_offsets must not be NULL", out_offsets=None, H=2048, W=1024)
    refused(f, UNSUPPORTED, "1048576", H=2048, W=1024, max_runs=524289)
    refused(f, UNSUPPORTED, "max_runs", max_runs=524289)
    # the rules hold for an empty batch too; a valid empty batch is success without a launch, whatever the pointers
    refused(f, ARG, "connectivity", B=0, connectivity=6)
    refused(f, ARG, "reserved", B=0, reserved=(0, 1))
    refused(f, ARG, "16-byte aligned", B=0, out_bits=p + 8192 + 8)
    refused(f, ARG, "overlap", B=0, out_bits=p)
    refused(f, UNSUPPORTED, "1048576", B=0, H=2048, W=1024)
    refused(f, UNSUPPORTED, "max_runs", B=0, max_runs=524289)
    assert call(f, B=0)[0] == 0 and call(f, B=0, P=0)[0] == 0
    assert call(f, B=0, bits=None, bits_offsets=None, frames=None, image_index=None, out_offsets=None, workspace=None)[0] == 0
    assert call(f, B=0, out_bits=None, out_offsets=None, components=None, max_components=0)[0] == 0


def test_c_entry_refuses_overlapping_buffers():
    f = Fake()
    refused(f, ARG, "overlap", out_bits=f.p)                               # in place
    refused(f, ARG, "overlap", out_bits=f.p + 4 * 60)                      # the last words of the input range
    refused(f, ARG, "overlap", bits=f.p + 8192 + 4 * 60)                   # the input begins inside the output range
    refused(f, ARG, "overlap", bits_words=4096, out_bits=f.p + 8192)       # a long input buffer that holds the output
    refused(f, ARG, "overlap", out_bits=f.p + 16)
    assert call(f, out_bits=f.p + 256, B=0)[0] == 0                        # side by side: [p, p + 256) and [p + 256, p + 512)


def test_c_entry_unsupported_sizes_at_the_edge_and_one_beyond():
    f = Fake()
    refused(f, UNSUPPORTED, "1048576", H=1024, W=1025)                     # 1024 * roundup32(1025) = 1024 * 1056
    refused(f, UNSUPPORTED, "1048576", H=1025, W=1024)
    refused(f, UNSUPPORTED, "1048576", H=32769, W=1)                       # 32769 rows of one word
    refused(f, UNSUPPORTED, "1048576", H=(1 << 31) - 1, W=(1 << 31) - 1)   # no 32-bit wrap
    refused(f, UNSUPPORTED, "max_runs", max_runs=524289)
    refused(f, UNSUPPORTED, "max_runs", max_runs=(1 << 31) - 1)
    # the documented bounds themselves pass the size rules: a valid empty batch, and with B > 0 the next rule speaks
    assert call(f, B=0, H=1024, W=1024)[0] == 0 and call(f, B=0, H=32768, W=1)[0] == 0 and call(f, B=0, H=1024, W=993)[0] == 0
    assert call(f, B=0, max_runs=524288)[0] == 0 and call(f, B=0, max_runs=65536)[0] == 0
    refused(f, ARG, "NULL", H=1024, W=1024, max_runs=524288, bits=None)


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


def test_python_argument_errors_come_before_any_device_work(monkeypatch):
    import torch

    import labelany3d_amd as la
    from labelany3d_amd import components

    class Reached:
        """stands in for the library: reaching the C entry, or sizing its workspace, fails the test"""

        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    monkeypatch.setattr(components, "lib", Reached())
    grid = host_grid(XC.SIZES)                                             # on the host: never reaches a device
    fb = host_bits(grid, XC.IMAGE_INDEX)
    planes = (la.components_bits_frames, la.largest_component_bits_frames, lambda fr, b, **kw: la.drop_islands_bits_frames(fr, b, 3, **kw))
    every = planes + (la.components_stats_frames,)
    # 1  a wrong frames type
    for fn in every:
        for fr in (grid.table_host, grid.table, None, (grid.table, grid.H, grid.W)):
            with pytest.raises(ValueError, match="frames must be"):
                fn(fr, fb)
    # 2  a foreign table, or no FrameBits at all
    other = host_grid(XC.SIZES[:-1] + ((32, 161),))
    for fn in every:
        with pytest.raises(ValueError, match="another frame table"):
            fn(other, fb)
        with pytest.raises(ValueError, match="must be the FrameBits"):
            fn(grid, (fb.bits, fb.offsets))
        with pytest.raises(ValueError, match="must be the FrameBits"):
            fn(grid, la.MaskBits(fb.bits.view(1, -1), 8, 32, 32))
    # 3  the scalars, with the messages of the uniform functions
    for fn in (la.components_bits_frames, la.components_stats_frames):
        for v in (-1, 2.0, True, "3", None):
            with pytest.raises(ValueError, match="min_area must be"):
                fn(grid, fb, min_area=v)
        for v in (2, -1, 1.0, "yes", None):
            with pytest.raises(ValueError, match="largest must be"):
                fn(grid, fb, largest=v)
        for v in (0, 6, 9, 8.0, True, "8", None):
            with pytest.raises(ValueError, match="connectivity must be"):
                fn(grid, fb, connectivity=v)
        for v in (-1, 1.5, True, None):
            with pytest.raises(ValueError, match="max_components must be"):
                fn(grid, fb, max_components=v)
        for v in (0, -1, 524289, 1 << 40, 16384.0, True, None):
            with pytest.raises(ValueError, match="max_runs must be"):
                fn(grid, fb, max_runs=v)
    for v in (-1, 2.0, None):
        with pytest.raises(ValueError, match="min_area must be"):
            la.drop_islands_bits_frames(grid, fb, v)
    with pytest.raises(TypeError):
        la.drop_islands_bits_frames(grid, fb)                               # min_area has no default there
    with pytest.raises(ValueError, match="connectivity must be"):
        la.largest_component_bits_frames(grid, fb, connectivity=6)
    with pytest.raises(ValueError, match="max_runs must be"):
        la.largest_component_bits_frames(grid, fb, max_runs=0)
    big = host_grid([(1025, 1024)])
    with pytest.raises(ValueError, match="1048576 pixels"):
        la.components_stats_frames(big, host_bits(big, [0]))
    # 4  a bad out: not flat, another dtype, too short, on the host, overlapping
    n = fb.bits.numel()
    for fn in planes:
        for out in (torch.zeros((2, n), dtype=torch.int32), torch.zeros(n, dtype=torch.int64), torch.zeros(n - 1, dtype=torch.int32),
                    torch.zeros(n, dtype=torch.int32), torch.zeros(2 * n, dtype=torch.int32)[::2], np.zeros(n, np.int32), "out"):
            with pytest.raises(ValueError, match="out must be"):
                fn(grid, fb, out=out)
        for out in (fb.bits, fb.bits[4:], fb.bits[:8]):
            with pytest.raises(ValueError, match="overlaps"):
                fn(grid, fb, out=out)
    # the last check of all: where the planes live
    for fn in every:
        with pytest.raises(ValueError, match="on the GPU"):
            fn(grid, fb)
