"""CPU-only tests of connected components on bit planes (include/la3d.h "connected components on bit planes"): the NumPy restatement
against what SciPy gave (tests/golden/g20_components.npz), the names on every layer, the layout of the argument block, the C entry's
refusals before any launch (fake pointers: nothing here reaches a device), the workspace bound and the Python argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import components_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def g():
    return CC.load_golden()


def test_restatement_equals_the_fixture(g):
    """what SciPy gave when the fixture was made, on every fixture case - the three 480 x 640 planes included"""
    np.testing.assert_array_equal(g["frames"], CC.FIXTURE_FRAMES)
    small, big = CC.fixture_planes(), CC.big_planes()
    for f, planes in enumerate(small):
        np.testing.assert_array_equal(CC.unpack(g[f"in_{f}"], *CC.FIXTURE_FRAMES[f]), planes)
    runs = [CC.count_runs(m) for m in big]
    assert runs == g["big_runs"].tolist() and all(6200 <= r <= 6600 for r in runs), runs
    labelled = {}
    changed = 0
    for key, f, p, conn, min_area, largest in CC.fixture_keys():
        mask = big[p] if f < 0 else small[f][p]
        if (f, p, conn) not in labelled:
            labels, n = CC.label(mask, conn)
            labelled[f, p, conn] = labels, n, CC.table_of(labels, n)
        labels, n, table = labelled[f, p, conn]
        out, stats = CC.choose(labels, n, table, min_area, largest)
        np.testing.assert_array_equal(stats, g[f"stats_{key}"], err_msg=key)
        tab = np.zeros((CC.TABLE_ROWS, 5), np.int32)
        tab[:min(n, CC.TABLE_ROWS)] = table[:CC.TABLE_ROWS]
        np.testing.assert_array_equal(tab, g[f"table_{key}"], err_msg=key)
        if f < 0:
            assert 2000 <= n <= 5000, (key, n)
            assert CC.words_sha256(out, CC.BIG_FRAME[1]) == bytes(g[f"sha_{key}"]).hex(), key
        else:
            H, W = CC.FIXTURE_FRAMES[f]
            np.testing.assert_array_equal(out, CC.unpack(g[f"out_{key}"][None], H, W)[0], err_msg=key)
        changed += bool(out.any()) and not np.array_equal(out, mask)
    assert 2 * changed >= len(CC.fixture_keys()), changed       # the fixture is not made of planes that come back as they went in
    assert os.path.getsize(CC.GOLDEN) < 128 * 1024


def test_case_lists_cover_what_they_promise():
    cases = CC.all_cases()
    names = [n for n, _ in cases]
    assert len(set(names)) == len(names)
    assert max(CC.count_runs(m) for _, m in cases) <= CC.MAX_CASE_RUNS
    for H, W in CC.frames():
        assert sum(n.endswith(f"_{H}x{W}") for n in names) >= 8, (H, W)
    for pat, _ in CC.PATTERNS:
        assert sum(n.startswith(pat + "_") for n in names) >= 8, pat
    by = dict(cases)
    # the patterns do what their names say
    assert CC.label(by["spiral_96x224"], 4)[1] == 1 and CC.label(by["spiral_33x47"], 8)[1] == 1
    assert CC.label(by["comb_33x47"], 4)[1] == 1
    assert CC.label(by["checkerboard_33x47"], 8)[1] == 1 and CC.label(by["checkerboard_33x47"], 4)[1] == (33 * 47 + 1) // 2
    d = by["diagonals_33x47"]
    assert CC.label(d, 4)[1] == int(d.sum()) and CC.label(d, 8)[1] < 33 + 47
    assert CC.label(by["ring_33x47"], 8)[1] == 2
    s = by["seams_33x47"]
    assert CC.label(s, 8)[1] == CC.label(s, 4)[1] == int(s.sum()) - 1      # only the 31 | 32 pair is joined
    e = by["equal_pair_33x47"]
    out, stats, tab = CC.components(e, 8, 0, True, 4)
    assert stats[0] == 2 and tab[0, 0] == tab[1, 0] and stats[1] == 1 and out[0, 46] and not out[32, 0]
    a = by["area_steps_33x47"]
    assert CC.components(a, 8, CC.MIN_AREA, False)[1][:2].tolist() == [5, 3]
    assert {n.split("_")[1] for n in names if n.startswith("random_")} == {str(x) for x in CC.DENSITIES}


def test_restatement_equals_scipy_on_every_case():
    ndi = pytest.importorskip("scipy.ndimage")
    structure = {4: ndi.generate_binary_structure(2, 1), 8: np.ones((3, 3), int)}
    for name, m in CC.all_cases():
        for conn in (4, 8):
            want, n = ndi.label(m, structure[conn])
            got, k = CC.label(m, conn)
            assert k == n and np.array_equal(got, want), (name, conn)


def test_names_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _lib, components

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    assert "connected components on bit planes" in hdr
    assert re.search(r"\bsize_t la3d_components_workspace_bytes\s*\(", hdr) and re.search(r"\bint la3d_components_bits\s*\(", hdr)
    for fn in ("la3d_components_bits", "la3d_components_workspace_bytes"):
        assert fn in _lib.EXPORTS and hasattr(_lib.lib, fn), fn
    for fn in ("components_bits", "components_stats", "largest_component_bits", "drop_islands_bits"):
        assert callable(getattr(la, fn)) and fn in la.__all__ and getattr(components, fn) is getattr(la, fn), fn
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2     # additive
    from labelany3d_amd import _build
    assert any(s.endswith("la3d_components.hip") for s in _build.SOURCES)


def test_block_layout_matches_the_header():
    """the ctypes block against the header's text: the same fields in the same order with the same types, and the natural offsets"""
    from labelany3d_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    body = re.search(r"typedef struct la3d_components_args \{(.*?)\} la3d_components_args;", hdr, re.S).group(1)
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
            want.append((nm.strip(), C.c_void_p if star else ctype[base]))
    assert [(n, t) for n, t in _lib.ComponentsArgs._fields_] == want
    off = 0
    for n, t in want:
        off = (off + C.alignment(t) - 1) // C.alignment(t) * C.alignment(t)
        assert getattr(_lib.ComponentsArgs, n).offset == off, n
        off += C.sizeof(t)
    assert C.sizeof(_lib.ComponentsArgs) == 104 == (off + 7) // 8 * 8
    assert _lib.ComponentsArgs.mask_bits.offset == 40 and _lib.ComponentsArgs.stream.offset == 96


class Fake:
    """fake "device" memory, 64-byte aligned: every call below is refused, or has nothing to do, before any launch"""

    def __init__(self):
        self.buf = (C.c_char * 32768)()
        self.p = (C.addressof(self.buf) + 63) & ~63


def call(f, size=None, **kw):
    from labelany3d_amd import _lib

    a = dict(B=2, H=8, W=32, frame_width=0, connectivity=8, min_area=0, largest=0, max_runs=64, max_components=4,
             mask_bits=f.p, bits_plane_stride=8, out_bits=f.p + 4096, out_plane_stride=8, stats=f.p + 8192, components=f.p + 12288,
             workspace=f.p + 16384, stream=None)
    a.update(kw)
    blk = _lib.ComponentsArgs(struct_size=C.sizeof(_lib.ComponentsArgs) if size is None else size, **a)
    rc = _lib.lib.la3d_components_bits(C.byref(blk))
    return rc, _lib.lib.la3d_last_error()


def refused(f, code, word, **kw):
    rc, msg = call(f, **kw)
    assert rc == code and word.encode() in msg and msg.startswith(b"la3d_components_bits: "), (kw, rc, msg)


def test_c_entry_refuses_before_any_launch():
    from labelany3d_amd import _lib

    f = Fake()
    for size in (0, 96, 103, 105, 112, -1):
        refused(f, ARG, "struct_size", size=size)
    assert _lib.lib.la3d_components_bits(None) == ARG
    for kw in (dict(B=-1), dict(H=0), dict(W=0), dict(H=-3), dict(W=-1)):
        refused(f, ARG, "B >= 0, H, W > 0", **kw)
    for fw in (-1, 33, 1 << 20):
        refused(f, ARG, "frame_width", frame_width=fw)
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
    refused(f, ARG, "NULL", mask_bits=None)
    refused(f, ARG, "NULL", workspace=None)
    for name, base in (("mask_bits", 0), ("out_bits", 4096), ("stats", 8192), ("components", 12288), ("workspace", 16384)):
        for d in (1, 2, 3):
            refused(f, ARG, "4-byte aligned", **{name: f.p + base + d})
    refused(f, ARG, "bits_plane_stride", bits_plane_stride=7)
    refused(f, ARG, "out_plane_stride", out_plane_stride=7)
    refused(f, ARG, "bits_plane_stride", H=9, W=33, bits_plane_stride=9)     # 297 bits: 10 words
    # the rank: the first rule that fails speaks
    refused(f, ARG, "struct_size", size=8, B=-1)
    refused(f, ARG, "B >= 0", B=-1, connectivity=5)
    refused(f, ARG, "frame_width", frame_width=40, connectivity=5)
    refused(f, ARG, "connectivity", connectivity=5, largest=2)
    refused(f, ARG, "largest", largest=2, min_area=-1)
    refused(f, ARG, "min_area", min_area=-1, max_runs=0)
    refused(f, ARG, "max_runs", max_runs=0, max_components=-1)
    refused(f, ARG, "nothing to do", out_bits=None, stats=None, components=None, H=2048, W=1024)
    refused(f, UNSUPPORTED, "1048576", H=2048, W=1024, mask_bits=None)
    # the rules hold for an empty batch too; a valid empty batch is success without a launch, whatever the pointers
    refused(f, ARG, "connectivity", B=0, connectivity=6)
    refused(f, UNSUPPORTED, "max_runs", B=0, max_runs=524289)
    assert call(f, B=0)[0] == 0
    assert call(f, B=0, mask_bits=None, workspace=None, out_bits=None, components=None, max_components=0)[0] == 0
    assert call(f, B=0, mask_bits=f.p + 1, out_bits=f.p)[0] == 0


def test_c_entry_refuses_overlapping_planes():
    f = Fake()
    refused(f, ARG, "overlap", out_bits=f.p)                                # in place
    refused(f, ARG, "overlap", out_bits=f.p + 4 * 15)                       # the last word of the input range
    refused(f, ARG, "overlap", mask_bits=f.p + 4096 + 4 * 15)               # the input begins inside the output range
    refused(f, ARG, "overlap", bits_plane_stride=600, out_bits=f.p + 2048)  # long strides: planes of one lie between planes of the other
    refused(f, ARG, "overlap", bits_plane_stride=0, out_plane_stride=0, out_bits=f.p + 4 * 15)   # stride 0 = the words of a plane


def test_c_entry_unsupported_sizes():
    f = Fake()
    refused(f, UNSUPPORTED, "1048576", H=1024, W=1025, bits_plane_stride=1 << 20, out_plane_stride=1 << 20)
    refused(f, UNSUPPORTED, "1048576", H=1048577, W=1, bits_plane_stride=1 << 20, out_plane_stride=1 << 20)
    refused(f, UNSUPPORTED, "max_runs", max_runs=524289)
    refused(f, UNSUPPORTED, "max_runs", max_runs=(1 << 31) - 1)
    # 65536 and the documented bound itself pass the size rules (the next rule speaks)
    refused(f, ARG, "NULL", max_runs=65536, mask_bits=None)
    refused(f, ARG, "NULL", max_runs=524288, mask_bits=None)
    refused(f, ARG, "NULL", H=1024, W=1024, mask_bits=None)


def test_workspace_bound_holds():
    from labelany3d_amd import _lib

    ws = _lib.lib.la3d_components_workspace_bytes
    assert ws(0, 480, 16384) == 0 and ws(4, 0, 16384) == 0 and ws(4, 480, 0) == 0 and ws(-1, 480, 64) == 0 and ws(1, -1, 64) == 0
    for B in (1, 2, 65, 1024, 1 << 20):
        for H in (1, 33, 480, 1 << 20):
            for mr in (1, 64, 16384, 65536, 524288):
                got = ws(B, H, mr)
                assert 0 < got <= B * (16 * mr + 8 * H) + 4096, (B, H, mr, got)
                assert got >= B * (8 * mr + 4 * (H + 1))                   # a run's two ends and a row's first run at the least
    assert ws(1 << 20, 1 << 20, 524288) > 1 << 32                          # size_t: no 32-bit wrap
    sizes = [ws(B, 480, 16384) for B in (1, 2, 16, 300, 1024)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]


def test_python_argument_errors_come_before_any_device_work():
    import torch

    import labelany3d_amd as la

    mb = la.MaskBits(torch.zeros((2, 8), dtype=torch.int32), 8, 32, 32)     # on the host: never reaches a device
    forms = (la.components_bits, la.components_stats)
    for fn in forms:
        for v in (-1, 2.0, True, "3", None):
            with pytest.raises(ValueError, match="min_area must be"):
                fn(mb, min_area=v)
        for v in (2, -1, 1.0, "yes", None):
            with pytest.raises(ValueError, match="largest must be"):
                fn(mb, largest=v)
        for v in (0, 6, 9, 8.0, True, "8", None):
            with pytest.raises(ValueError, match="connectivity must be"):
                fn(mb, connectivity=v)
        for v in (-1, 1.5, True, None):
            with pytest.raises(ValueError, match="max_components must be"):
                fn(mb, max_components=v)
        for v in (0, -1, 524289, 1 << 40, 16384.0, True, None):
            with pytest.raises(ValueError, match="max_runs must be"):
                fn(mb, max_runs=v)
        with pytest.raises(ValueError, match="must be a MaskBits"):
            fn((mb.bits, 8, 32, 32))
        with pytest.raises(ValueError, match="must be a MaskBits"):
            fn(mb.bits)
        with pytest.raises(ValueError, match="on the GPU"):
            fn(mb)
        with pytest.raises(ValueError, match="frame_width"):
            fn(la.MaskBits(mb.bits, 8, 32, 33))
        with pytest.raises(ValueError, match="empty frame"):
            fn(la.MaskBits(torch.zeros((2, 0), dtype=torch.int32), 0, 32, 32))
        with pytest.raises(ValueError, match="1048576 pixels"):
            fn(la.MaskBits(mb.bits, 2048, 1024, 1024))
    for v in (-1, 2.0, None):
        with pytest.raises(ValueError, match="drop_islands_bits|min_area must be"):
            la.drop_islands_bits(mb, v)
    with pytest.raises(TypeError):
        la.drop_islands_bits(mb)                                            # min_area has no default there
    with pytest.raises(ValueError, match="connectivity must be"):
        la.largest_component_bits(mb, connectivity=6)
    with pytest.raises(ValueError, match="max_runs must be"):
        la.largest_component_bits(mb, max_runs=0)
    with pytest.raises(ValueError, match="on the GPU"):
        la.largest_component_bits(mb)
