"""CPU-only contract of the annotation bit-plane packers (include/la3d.h "annotations as bit planes": ``la3d_pack_rle_bits``,
``la3d_pack_poly_bits`` and their frames forms): the exports exist on every layer, the argument blocks keep their pinned sizes, the C
entries refuse before any launch (fake pointers: nothing below reaches a device), and the Python argument errors come before any
device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_C = ("la3d_pack_rle_bits", "la3d_pack_poly_bits", "la3d_pack_rle_bits_frames", "la3d_pack_poly_bits_frames")
NEW_PY = ("pack_rle_bits", "pack_poly_bits", "pack_rle_bits_frames", "pack_poly_bits_frames")
ARG, UNSUPPORTED = -1, -2


def test_exports_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _lib, frames, masks

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    for fn in NEW_C:
        assert re.search(rf"\bint {fn}\s*\(", hdr), fn
        assert fn in _lib.EXPORTS and hasattr(_lib.lib, fn), fn
    for fn in NEW_PY:
        assert callable(getattr(la, fn)) and fn in la.__all__, fn
        assert getattr(masks, fn) is getattr(la, fn)
    assert frames.pack_rle_bits_frames is la.pack_rle_bits_frames and frames.pack_poly_bits_frames is la.pack_poly_bits_frames
    assert "annotations as bit planes" in hdr
    # additive: the version and the pinned sizes of the argument blocks stay
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2
    assert C.sizeof(_lib.FitArgs) == 232 and C.sizeof(_lib.CloudArgs) == 192
    assert C.sizeof(_lib.Depth16Block) == 32 and C.sizeof(_lib.Frame) == 24


class Fake:
    """fake "device" memory, 64-byte aligned: every call below is refused, or has nothing to do, before any launch"""

    def __init__(self):
        self.buf = (C.c_char * 4096)()
        self.p = (C.addressof(self.buf) + 63) & ~63


def uniform_call(kind, f, **kw):
    from labelany3d_amd import _lib

    a = dict(src=f.p, src2=f.p + 1024, src3=f.p + 2048, B=2, H=8, W=32, W_out=32, bits=f.p + 3072, stride=8, area=f.p + 3584)
    a.update(kw)
    ann = (a["src"], a["src2"]) if kind == "rle" else (a["src"], a["src2"], a["src3"])
    fn = _lib.lib.la3d_pack_rle_bits if kind == "rle" else _lib.lib.la3d_pack_poly_bits
    return fn(*ann, a["B"], a["H"], a["W"], a["W_out"], a["bits"], a["stride"], a["area"], None), _lib.lib.la3d_last_error()


def frames_call(kind, f, **kw):
    from labelany3d_amd import _lib

    a = dict(src=f.p, src2=f.p + 512, src3=f.p + 1024, frames=f.p + 1536, P=1, H=8, W=32, ii=f.p + 2048, B=2, bits=f.p + 3072,
             offs=f.p + 2560, area=f.p + 3584)
    a.update(kw)
    ann = (a["src"], a["src2"]) if kind == "rle" else (a["src"], a["src2"], a["src3"])
    fn = _lib.lib.la3d_pack_rle_bits_frames if kind == "rle" else _lib.lib.la3d_pack_poly_bits_frames
    return fn(*ann, a["frames"], a["P"], a["H"], a["W"], a["ii"], a["B"], a["bits"], a["offs"], a["area"], None), _lib.lib.la3d_last_error()


UNIFORM_REFUSALS = [
    ("negative B", dict(B=-1), ARG),
    ("empty H", dict(H=0), ARG),
    ("negative H", dict(H=-8), ARG),
    ("negative W", dict(W=-32), ARG),
    ("W_out < W", dict(W_out=31), ARG),
    ("W_out no multiple of 32", dict(W=30, W_out=31), ARG),
    ("NULL annotations", dict(src=None), ARG),
    ("NULL offsets", dict(src2=None), ARG),
    ("NULL bits", dict(bits=None), ARG),
    ("misaligned bits", dict(bits="bits+2"), ARG),
    ("misaligned area", dict(area="area+2"), ARG),
    ("stride below a plane", dict(stride=7), ARG),
    ("stride below a padded plane", dict(W=33, W_out=64, stride=15), ARG),
    ("frame beyond LDS", dict(H=1025, W=1024, W_out=1024, stride=1 << 20), UNSUPPORTED),
]


@pytest.mark.parametrize("kind", ["rle", "poly"])
@pytest.mark.parametrize("name,kw,code", UNIFORM_REFUSALS, ids=[r[0] for r in UNIFORM_REFUSALS])
def test_uniform_entries_refuse_before_any_launch(kind, name, kw, code):
    f = Fake()
    base = dict(bits=f.p + 3072, area=f.p + 3584)
    kw = {k: (base[v.split("+")[0]] + int(v.split("+")[1]) if isinstance(v, str) else v) for k, v in kw.items()}
    rc, err = uniform_call(kind, f, **kw)
    assert rc == code, (name, err)
    assert (b"la3d_pack_rle_bits" if kind == "rle" else b"la3d_pack_poly_bits") in err


FRAMES_REFUSALS = [
    ("negative B", dict(B=-1), ARG),
    ("negative P", dict(P=-1), ARG),
    ("empty bounds", dict(H=0), ARG),
    ("negative bounds", dict(W=-1), ARG),
    ("NULL annotations", dict(src=None), ARG),
    ("NULL frames", dict(frames=None), ARG),
    ("NULL image_index", dict(ii=None), ARG),
    ("NULL bits", dict(bits=None), ARG),
    ("NULL bits_offsets", dict(offs=None), ARG),
    ("bits not 16-byte aligned", dict(bits="bits+4"), ARG),
    ("misaligned frames", dict(frames="frames+4"), ARG),
    ("misaligned bits_offsets", dict(offs="offs+4"), ARG),
    ("misaligned image_index", dict(ii="ii+2"), ARG),
    ("bounds beyond LDS", dict(H=1025, W=1000), UNSUPPORTED),
]


@pytest.mark.parametrize("kind", ["rle", "poly"])
@pytest.mark.parametrize("name,kw,code", FRAMES_REFUSALS, ids=[r[0] for r in FRAMES_REFUSALS])
def test_frames_entries_refuse_before_any_launch(kind, name, kw, code):
    f = Fake()
    base = dict(bits=f.p + 3072, frames=f.p + 1536, offs=f.p + 2560, ii=f.p + 2048)
    kw = {k: (base[v.split("+")[0]] + int(v.split("+")[1]) if isinstance(v, str) else v) for k, v in kw.items()}
    rc, err = frames_call(kind, f, **kw)
    assert rc == code, (name, err)
    assert (b"la3d_pack_rle_bits_frames" if kind == "rle" else b"la3d_pack_poly_bits_frames") in err


@pytest.mark.parametrize("kind", ["rle", "poly"])
def test_an_empty_batch_succeeds_without_a_launch(kind):
    f = Fake()
    assert uniform_call(kind, f, B=0)[0] == 0
    assert uniform_call(kind, f, B=0, src=None, src2=None, src3=None, bits=None, area=None)[0] == 0
    assert frames_call(kind, f, B=0)[0] == 0
    assert frames_call(kind, f, B=0, src=None, src2=None, src3=None, frames=None, ii=None, bits=None, offs=None, area=None)[0] == 0


# ---- Python: every argument error comes before any device work (no GPU is visible to these tests) -------------------------------
def _rle(h, w, counts=(3, 4)):
    return {"size": [h, w], "counts": list(counts) + [h * w - sum(counts)]}


def _host_frames(la, sizes):
    return la.pack_frames([np.ones(s, np.float32) for s in sizes], device="cpu")


def test_python_argument_errors_uniform():
    import torch

    import labelany3d_amd as la

    with pytest.raises(ValueError, match="share the frame size"):
        la.pack_rle_bits([_rle(8, 32), _rle(8, 64)])
    with pytest.raises(ValueError, match="empty frame"):
        la.pack_rle_bits((np.zeros(2, np.int32), np.array([0, 2], np.int64), 0, 32))
    with pytest.raises(ValueError, match="bit planes must be an int32 tensor"):
        la.pack_rle_bits([_rle(8, 32)], out=torch.zeros((1, 8), dtype=torch.int32))          # a host tensor
    with pytest.raises(ValueError, match="area must be"):
        la.pack_rle_bits([_rle(8, 32)], area=torch.zeros(1, dtype=torch.int32))
    polys = la.pack_polygons([[[1, 1, 20, 1, 10, 6]]], 8, 32)
    with pytest.raises(ValueError, match="tuple of pack_polygons"):
        la.pack_poly_bits([[[1, 1, 20, 1, 10, 6]]])
    with pytest.raises(ValueError, match="bit planes must be an int32 tensor"):
        la.pack_poly_bits(polys, out=torch.zeros((1, 8), dtype=torch.int32))
    with pytest.raises(ValueError, match="area must be"):
        la.pack_poly_bits(polys, area=np.zeros(1, np.int32))
    with pytest.raises(ValueError, match="empty frame"):
        la.pack_poly_bits(polys[:3] + (8, 0))


def test_python_argument_errors_frames():
    import labelany3d_amd as la

    pf = _host_frames(la, [(8, 32), (5, 13)])
    rles = [_rle(8, 32), _rle(5, 13), _rle(8, 32)]
    polys = la.pack_polygons([[[1, 1, 20, 1, 10, 6]], [[0, 0, 5, 0, 5, 4]], []], 1, 1)
    for fn, ann in ((la.pack_rle_bits_frames, rles), (la.pack_poly_bits_frames, polys)):
        with pytest.raises(ValueError, match="PackedFrames"):
            fn((pf.depth, pf.table), ann, [0, 1, 0])
        with pytest.raises(ValueError, match="image_index is required"):
            fn(pf, ann, None)
        with pytest.raises(ValueError, match="one image per annotation"):
            fn(pf, ann, [0, 1])
        with pytest.raises(ValueError, match=r"must lie in \[0, 2\)"):
            fn(pf, ann, [0, 1, 2])
        with pytest.raises(ValueError, match=r"must lie in \[0, 2\)"):
            fn(pf, ann, [0, -1, 0])
        with pytest.raises(ValueError, match="must be integers"):
            fn(pf, ann, [0.0, 1.0, 0.5])
        with pytest.raises(ValueError, match="must live on the GPU"):                        # the table of a host layout
            fn(pf, ann, [0, 1, 0])
    with pytest.raises(ValueError, match="size differs from the size of its image"):
        la.pack_rle_bits_frames(pf, rles, [0, 0, 0])
    with pytest.raises(ValueError, match="tuple of pack_polygons"):
        la.pack_poly_bits_frames(pf, [[[1, 1, 20, 1, 10, 6]]], [0])
