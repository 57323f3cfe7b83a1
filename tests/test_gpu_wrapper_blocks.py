"""What the Python wrappers of the depth + mask fit send to the library: which C entry every call reaches, and with which
``la3d_fit_args`` block.  The records themselves are held to the oracle by the rest of the GPU suite; this module pins the part no
other test sees.  Six attributes of ``labelany3d_amd._lib.lib`` are replaced with spies that record and then forward
(``la3d_fit_instances_ex`` / ``_bits`` / ``_depth16`` / ``_frames`` / ``_frames_depth16`` and ``la3d_fit_annotations_host``: the
wrappers look them up on that object at call time).  Per C call the recording holds the entry name, every non-pointer field of the
block by value, for every pointer field except ``stream`` whether it is NULL, whether the depth planes / bit planes are the
caller's own tensor (fitted where they lie) or a copy padded by the wrapper, the scalars of the ``la3d_depth16`` block, the
bit-plane stride and flags, and the frame count.  Per case it also holds the shapes of what the wrapper returned (a B = 0 call
records no C call at all).  ``tests/golden/wrapper_blocks.json`` is that recording taken with the Python layer as it was before the
wrappers were rebuilt on one call builder (``tests/golden/make_golden_wrapper_blocks.py``); the comparison is field for field and
call for call."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

from oracle import la3d_oracle as O

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wrapper_blocks.json")
ENTRIES = ("la3d_fit_instances_ex", "la3d_fit_instances_bits", "la3d_fit_instances_depth16", "la3d_fit_instances_frames",
           "la3d_fit_instances_frames_depth16", "la3d_fit_annotations_host")
B, H, P = 5, 24, 2
IMG = np.array([0, 1, 1, 0, 1], np.int32)
K3 = np.array([[60.0, 0, 30], [0, 60.0, 12], [0, 0, 1]])
FRAME_SIZES = [(24, 50), (16, 64), (9, 33)]
FLT = {"boundary_threshold": 2, "scale_threshold": 20}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def rects(W):
    """(B,H,W) bool: four rectangles (one of more than 500 pixels, so that subsample mode draws) and an empty plane"""
    m = np.zeros((B, H, W), bool)
    m[0, 2:23, 3:3 + 40] = True
    m[1, 5:15, 10:30] = True
    m[2, 1:20, W - 14:W - 2] = True
    m[4, 8:22, 20:45] = True
    return m


def rect_polys(W):
    """the same five instances as polygon part lists (the empty one: no part)"""
    box = lambda r0, r1, c0, c1: [[c0, r0, c1, r0, c1, r1, c0, r1]]   # noqa: E731
    return [box(2, 22, 3, 42), box(5, 14, 10, 29), box(1, 19, W - 14, W - 3), [], box(8, 21, 20, 44)]


def depth_planes(n, h, w, seed=0):
    vv, uu = np.mgrid[0:h, 0:w]
    return (2.0 + 0.01 * uu + 0.02 * vv + 0.03 * np.random.RandomState(seed).rand(n, h, w)).astype(np.float32)


def ground_rows(n):
    return np.array([[0.05, -0.97, 0.1, 1.2]] * n) + 0.01 * np.random.RandomState(3).randn(n, 4)


def draws(la, masks):
    return la.draw_sample_idx(masks.reshape(len(masks), -1).sum(1), rng=np.random.RandomState(1))


def annotations(W, with_area=True):
    """eight annotations of one 24 x W image: both kinds of segmentation, a crowd one and one without a segmentation"""
    m, polys, out = rects(W), rect_polys(W), []
    for n in (0, 1, 2, 4):
        out.append({"segmentation": O.rle_encode(m[n]), "bbox": [0, 0, 1, 1], "category_id": n + 1, "iscrowd": 0})
        out.append({"segmentation": polys[n], "bbox": [1, 1, 2, 2], "category_id": n + 11, "iscrowd": 0})
    out[2]["iscrowd"] = 1
    del out[5]["segmentation"]
    if with_area:
        for a, n in zip(out, (0, 0, 1, 1, 2, 2, 4, 4)):
            a["area"] = float(m[n].sum())
    return out


class Own:
    """the tensors of a call that are the caller's own: the spy says whether the library was handed exactly these"""

    def __init__(self, depth=None, bits=None):
        d = depth
        if isinstance(d, tuple):          # (PackedFrames.depth / PackedFrames16.data / Depth16.data)
            d = d.depth if hasattr(d, "depth") else d.data
        self.depth = d.data_ptr() if hasattr(d, "data_ptr") and d.is_cuda else None
        self.bits = bits.data_ptr() if bits is not None else None


# ---- the cases: name -> function(la, torch) -> (thunk, Own) ------------------------------------------------------------------------
def _depth_given(la, torch, W, kind, padded):
    """(depth argument, frame_width argument) of a call on a 24 x W frame: float32 / Depth16 planes at the frame width, or already
    padded with an explicit frame_width"""
    d = torch.as_tensor(depth_planes(P, H, W), device="cuda")
    if kind == "f32":
        return (la.pad_depth_rows(d)[0], W) if padded else (d, None)
    return (la.pack_depth16(d, kind, frame_pad=True), W) if padded else (la.pack_depth16(d, kind), None)


def _ex_case(src, W, kind, padded, **opt):
    def make(la, torch):
        depth, fw = _depth_given(la, torch, W, kind, padded)
        m = rects(W)
        kw = dict(image_index=IMG, frame_width=fw)
        if src == "u8":
            kw["masks"] = m
            del kw["frame_width"]
        elif src == "rle":
            kw["rles"] = [O.rle_encode(x) for x in m]
        else:
            kw["polys"] = la.pack_polygons(rect_polys(W), H, W)
        kw.update(_options(la, m, W, **opt))
        return (lambda: la.fit_instances_ex(depth, K3, **kw)), Own(depth)
    return make


def _options(la, m, W, ground=False, sample=False, filter=False, size=False, hint=False, hull=False):
    kw = {}
    if ground:
        kw["ground"] = ground_rows(len(m))
    if sample:
        kw["sample_idx"] = draws(la, m)
    if filter:
        kw["filter"] = FLT
    if size:
        kw["image_size"] = (W, H)
    if hint:
        kw["area_hint"] = m.reshape(len(m), -1).sum(1).astype(np.int32)
    if hull:
        kw["method"] = "convex_hull"
    return kw


def _bits_case(W, kind, padded, explicit=False, **opt):
    def make(la, torch):
        depth, _ = _depth_given(la, torch, W, kind, padded)
        m = rects(W)
        mb = la.pack_mask_bits(torch.as_tensor(m, device="cuda"))
        kw = dict(image_index=IMG, **_options(la, m, W, **opt))
        if explicit:
            kw.update(frame_width=W, height_rule="span")
        return (lambda: la.fit_instances_bits(depth, mb, K3, **kw)), Own(depth, mb.bits)
    return make


def _fitter_case(bits, kind):
    def make(la, torch):
        W = 64
        m = rects(W)
        d = torch.as_tensor(depth_planes(P, H, W), device="cuda")
        depth = d if kind == "f32" else la.pack_depth16(d, kind)
        f = la.InstanceFitter(B, H, W)
        k = torch.as_tensor(np.stack([K3, K3]), device="cuda")
        ii, g = torch.as_tensor(IMG, device="cuda"), torch.as_tensor(ground_rows(B), device="cuda")
        mt = torch.as_tensor(m, device="cuda").view(torch.uint8)
        if not bits:
            return (lambda: f.run(depth, mt, k, ground=g, image_index=ii)), Own(depth)
        mb = la.pack_mask_bits(mt)
        if bits == "tuple":
            return (lambda: f.run_bits(depth, mb, k, ground=g, image_index=ii, height_rule="span")), Own(depth, mb.bits)
        return (lambda: f.run_bits(depth, mb.bits, k, image_index=ii, frame_width=60)), Own(depth, mb.bits)
    return make


def _u8_case(W, kind, **kw):
    def make(la, torch):
        d = torch.as_tensor(depth_planes(P, H, W), device="cuda")
        depth = d if kind == "f32" else la.pack_depth16(d, kind)
        return (lambda: la.fit_instances(depth, rects(W), K3, image_index=IMG, **kw)), Own(depth)
    return make


def _frames_mix():
    """six instances on three images of different sizes (one of them empty), as masks of each image's own size"""
    img = np.array([0, 0, 1, 2, 1, 2], np.int32)
    masks = []
    for n, p in enumerate(img):
        h, w = FRAME_SIZES[p]
        m = np.zeros((h, w), bool)
        if n != 4:
            m[1 + n % 3:h - 2, 2 + n:w - 3 - n] = True
        masks.append(m)
    return img, masks


def _frames_case(dtype, poly, full=False, device_index=False, shared_K=True):
    def make(la, torch):
        img, masks = _frames_mix()
        maps = [depth_planes(1, h, w, seed=p)[0] for p, (h, w) in enumerate(FRAME_SIZES)]
        if dtype == "f16":
            maps = [x.astype(np.float16) for x in maps]
        elif dtype == "u16":
            maps = [np.rint(x / 0.001).astype(np.uint16) for x in maps]
        pf = la.pack_frames(maps, device="cuda", dtype=dtype)
        if poly:
            segs = [[] if not m.any() else [[float(np.nonzero(m.any(0))[0][0]), float(np.nonzero(m.any(1))[0][0]),
                                             float(np.nonzero(m.any(0))[0][-1]), float(np.nonzero(m.any(1))[0][0]),
                                             float(np.nonzero(m.any(0))[0][-1]), float(np.nonzero(m.any(1))[0][-1])]] for m in masks]
            src = dict(polys=la.pack_polygons(segs, 24, 64))
        else:
            src = dict(rles=[O.rle_encode(m) for m in masks])
        kw = {}
        if full:
            kw = dict(ground=ground_rows(len(img)), sample_idx=np.zeros((len(img), 500), np.int32), filter=FLT, proj=True,
                      area_hint=np.array([m.sum() for m in masks], np.int32))
        K = K3 if shared_K else np.stack([K3] * 3)
        ii = torch.as_tensor(img, device="cuda") if device_index else img
        return (lambda: la.fit_instances_frames(pf, K, image_index=ii, **src, **kw)), Own(pf)
    return make


def _ann_case(W, to_host, planes=1, ground=False, with_area=True, device_K=False, **thresholds):
    def make(la, torch):
        ann = annotations(W, with_area)
        d = torch.as_tensor(depth_planes(planes, H, W), device="cuda")
        depth = d[0] if planes == 1 else d
        kw = dict(to_host=to_host, **thresholds)   # (the default thresholds drop every instance of so small an image)
        if planes > 1:
            kw["image_index"] = np.arange(len(ann), dtype=np.int32) % planes
        if ground:
            kw["ground"] = ground_rows(len(ann))
        K = torch.as_tensor(K3, device="cuda") if device_K else K3
        return (lambda: la.fit_annotations(ann, (W, H), depth, K, **kw)), Own(depth)
    return make


def _ann_all_case(W, filter):
    def make(la, torch):
        ann = annotations(W)
        depth = torch.as_tensor(depth_planes(P, H, W), device="cuda")
        ii = np.arange(len(ann), dtype=np.int32) % P
        return (lambda: la.fit_annotations_all(ann, (W, H), depth, K3, ground=ground_rows(len(ann)), image_index=ii, filter=filter)), Own(depth)
    return make


def _labels_case(kind, **kw):
    def make(la, torch):
        W = 50
        lab = np.zeros((2, H, W), np.uint8)
        lab[0, 2:20, 3:30], lab[0, 5:22, 32:48], lab[1, 4:18, 10:40] = 1, 2, 3
        d = torch.as_tensor(depth_planes(2, H, W), device="cuda")
        depth = d if kind == "f32" else la.pack_depth16(d, kind, frame_pad=True)
        return (lambda: la.fit_instances_labels(depth, lab, [[1, 2], [3]], K3, **kw)), Own(depth)
    return make


def _empty_case(which):
    def make(la, torch):
        W = 64
        depth = torch.as_tensor(depth_planes(1, H, W), device="cuda")
        none = np.zeros(0, np.int32)
        if which == "ex_u8":
            return (lambda: la.fit_instances_ex(depth, K3, masks=np.zeros((0, H, W), bool))), Own(depth)
        if which == "ex_rle":
            return (lambda: la.fit_instances_ex(depth, K3, rles=(np.zeros(1, np.int32), np.zeros(1, np.int64), H, W), filter=True,
                                                image_size=(W, H))), Own(depth)
        if which == "ex_poly":
            return (lambda: la.fit_instances_ex(depth, K3, polys=la.pack_polygons([], H, W))), Own(depth)
        if which == "u8":
            return (lambda: la.fit_instances(depth, np.zeros((0, H, W), bool), K3)), Own(depth)
        if which == "bits":
            mb = la.MaskBits(torch.zeros((0, H * W // 32), dtype=torch.int32, device="cuda"), H, W, W)
            return (lambda: la.fit_instances_bits(depth, mb, K3, filter=True, image_size=(W, H))), Own(depth, mb.bits)
        if which == "frames":
            pf = la.pack_frames([depth_planes(1, h, w)[0] for h, w in FRAME_SIZES], device="cuda")
            return (lambda: la.fit_instances_frames(pf, K3, rles=(np.zeros(1, np.int32), np.zeros(1, np.int64)), image_index=none,
                                                    filter=True, proj=True)), Own(pf)
        if which == "annotations":
            return (lambda: la.fit_annotations([], (W, H), depth, K3)), Own(depth)
        if which == "annotations_host":
            return (lambda: la.fit_annotations([{"iscrowd": 1}], (W, H), depth, K3, to_host=True)), Own(depth)
        if which == "annotations_all":
            return (lambda: la.fit_annotations_all([{"iscrowd": 1}], (W, H), depth, K3)), Own(depth)
        assert which == "labels"
        return (lambda: la.fit_instances_labels(depth.expand(2, H, W).contiguous(), np.zeros((2, H, W), np.uint8), [[], []], K3)), Own(depth)
    return make


def _cases():
    c = {}
    depths = ("f32", "f16", "u16")
    for src, W, kind, padded in itertools.product(("rle", "poly"), (64, 50), depths, (False, True)):
        c[f"ex-{src}-W{W}-{kind}-{'padded' if padded else 'frame'}"] = _ex_case(src, W, kind, padded)
    for W, kind in itertools.product((64, 50), depths):
        c[f"ex-u8-W{W}-{kind}"] = _ex_case("u8", W, kind, False)
        c[f"u8-W{W}-{kind}"] = _u8_case(W, kind)
    c["u8-W50-f32-hull"] = _u8_case(50, "f32", method="convex_hull")
    c["u8-W50-f32-sampled"] = lambda la, torch: _u8_case(50, "f32", sample_idx=draws(la, rects(50)))(la, torch)
    options = ("ground", "sample", "filter", "size", "hint", "hull")
    for o in options:
        c[f"ex-rle-W50-f32-{o}"] = _ex_case("rle", 50, "f32", False, **{o: True})
    everything = {o: True for o in options}
    for src, kind in itertools.product(("rle", "poly"), ("f32", "u16")):
        c[f"ex-{src}-W50-{kind}-everything"] = _ex_case(src, 50, kind, False, **everything)
    c["ex-u8-W64-f32-options"] = _ex_case("u8", 64, "f32", False, ground=True, sample=True, size=True, hint=True, hull=True)
    c["ex-rle-W50-host-depth"] = lambda la, torch: (
        (lambda: la.fit_instances_ex(depth_planes(P, H, 50), np.stack([K3, K3]), rles=[O.rle_encode(x) for x in rects(50)], image_index=IMG)), Own())
    c["rle-filter-tuple"] = lambda la, torch: (
        (lambda: la.fit_instances_rle(depth_planes(B, H, 50), [O.rle_encode(x) for x in rects(50)], K3, filter=True)), Own())
    c["poly-filter-tuple"] = lambda la, torch: (
        (lambda: la.fit_instances_poly(depth_planes(1, H, 50)[0], la.pack_polygons(rect_polys(50), H, 50), K3, filter=FLT)), Own())
    for W, kind, padded in itertools.product((64, 50), depths, (False, True)):
        c[f"bits-W{W}-{kind}-{'stored' if padded else 'frame'}"] = _bits_case(W, kind, padded, explicit=padded)
    for o in options:
        c[f"bits-W50-f32-{o}"] = _bits_case(50, "f32", False, **{o: True})
    for kind in ("f32", "f16"):
        c[f"bits-W50-{kind}-everything"] = _bits_case(50, kind, False, explicit=True, **everything)
    for bits, kind in itertools.product((None, "tuple", "tensor"), ("f32", "f16", "u16")):
        c[f"fitter-{'run' if not bits else 'run_bits-' + bits}-{kind}"] = _fitter_case(bits, kind)
    for dtype, poly in itertools.product((None, "f16", "u16"), (False, True)):
        c[f"frames-{dtype or 'f32'}-{'poly' if poly else 'rle'}"] = _frames_case(dtype, poly)
    for dtype in (None, "u16"):
        c[f"frames-{dtype or 'f32'}-rle-everything"] = _frames_case(dtype, False, full=True, shared_K=False)
        c[f"frames-{dtype or 'f32'}-poly-everything-device-index"] = _frames_case(dtype, True, full=True, device_index=True)
    for W, to_host in itertools.product((64, 50), (False, True)):
        c[f"annotations-W{W}-{'host' if to_host else 'device'}"] = _ann_case(W, to_host)
        c[f"annotations-W{W}-{'host' if to_host else 'device'}-planes-ground"] = _ann_case(W, to_host, planes=2, ground=True)
    for W, to_host in itertools.product((64, 50), (False, True)):
        c[f"annotations-W{W}-{'host' if to_host else 'device'}-kept"] = _ann_case(W, to_host, boundary_threshold=1, scale_threshold=20)
    c["annotations-W50-host-no-area"] = _ann_case(50, True, with_area=False)
    c["annotations-W50-device-no-area"] = _ann_case(50, False, with_area=False)
    c["annotations-W50-host-asked-device-K"] = _ann_case(50, True, device_K=True)
    for W, flt in itertools.product((64, 50), (None, True, FLT)):
        c[f"annotations_all-W{W}-{'filter-' + type(flt).__name__ if flt else 'plain'}"] = _ann_all_case(W, flt)
    c["labels-f32"] = _labels_case("f32")
    c["labels-u16-everything"] = _labels_case("u16", ground=ground_rows(3), sample_idx=np.zeros((3, 500), np.int32), filter=FLT,
                                              image_size=(50, H), method="convex_hull", height_rule="span")
    for which in ("ex_u8", "ex_rle", "ex_poly", "u8", "bits", "frames", "annotations", "annotations_host", "annotations_all", "labels"):
        c[f"empty-{which}"] = _empty_case(which)
    return c


CASES = _cases()


# ---- the spy ----------------------------------------------------------------------------------------------------------------------
def _addr(x):
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    return x.value or 0


def _block(a):
    from labelany3d_amd._lib import FitArgs

    rec = {}
    for name, ctype in FitArgs._fields_:
        if name == "stream":
            continue
        v = getattr(a, name)
        rec[name] = bool(v) if ctype is C.c_void_p else v
    return rec


def _describe(entry, args, own):
    a = args[0]._obj
    rec = {"entry": entry, "block": _block(a)}
    rest = list(args[1:])
    planes = a.depth or 0
    if entry in ("la3d_fit_instances_depth16", "la3d_fit_instances_frames_depth16"):
        d16 = rest.pop(0)._obj
        rec["depth16"] = {"struct_size": d16.struct_size, "dtype": d16.dtype, "plane_stride": d16.plane_stride, "scale": d16.scale,
                          "flags": d16.flags, "planes": bool(d16.planes)}
        planes = d16.planes or 0
    rec["depth_is_callers"] = own.depth is not None and planes == own.depth
    if entry in ("la3d_fit_instances_bits", "la3d_fit_instances_depth16"):
        ptr, stride, flags = rest
        rec["bits"] = {"given": bool(_addr(ptr)), "stride": int(stride), "flags": int(flags),
                       "is_callers": own.bits is not None and _addr(ptr) == own.bits}
    elif entry in ("la3d_fit_instances_frames", "la3d_fit_instances_frames_depth16"):
        rec["frames"] = {"table": bool(_addr(rest[0])), "P": int(rest[1])}
    return rec


def _shapes(x):
    if isinstance(x, dict):
        return {k: _shapes(v) for k, v in x.items()}
    if hasattr(x, "shape") and hasattr(x, "dtype"):
        return [type(x).__module__.split(".")[0], str(x.dtype).replace("torch.", ""), list(x.shape)]
    if isinstance(x, (tuple, list)):
        return [_shapes(v) for v in x]
    return type(x).__name__


def record(name, setattr_):
    """run one case under the spies: {"calls": [...], "returns": shapes} - or the exception the wrapper raised"""
    import torch

    import labelany3d_amd as la
    from labelany3d_amd import _lib

    thunk, own = CASES[name](la, torch)
    calls = []

    def spy(entry, real):
        def f(*args):
            calls.append(_describe(entry, args, own))
            return real(*args)
        return f
    for entry in ENTRIES:
        setattr_(_lib.lib, entry, spy(entry, getattr(_lib.lib, entry)))
    try:
        out = {"calls": calls, "returns": _shapes(thunk())}
    except Exception as e:  # noqa: BLE001 - an exception is part of what a wrapper does with a case
        out = {"calls": calls, "raises": [type(e).__name__, str(e)]}
    torch.cuda.synchronize()
    return json.loads(json.dumps(out))


# ---- the test ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pinned():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_every_case(pinned):
    assert sorted(pinned) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_wrapper_sends_the_pinned_blocks(pinned, monkeypatch, name):
    got, want = record(name, monkeypatch.setattr), pinned[name]
    assert "raises" not in want, want   # (every pinned case is a call that goes through)
    assert len(got["calls"]) == len(want["calls"]), (got, want)
    for n, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g["entry"] == w["entry"], (n, g, w)
        for part in w:
            if isinstance(w[part], dict):
                diff = {k: (g[part].get(k), v) for k, v in w[part].items() if g[part].get(k) != v}
                assert not diff and set(g[part]) == set(w[part]), (n, part, diff)
        assert g == w, (n, g, w)
    if name.startswith("empty-"):
        assert got["calls"] == []
    assert got.get("returns") == want["returns"], (got.get("returns"), want["returns"])
