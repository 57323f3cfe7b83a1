"""Which engine fits a call (la3d.hip, fit_dispatch), one row per rule: on config-2-shaped inputs with random depth, the records and
status of a call are bit for bit those of the same call pinned to the engine the rule names, and - where that is not the instance
engine - its records differ from those of the call pinned to the instance engine (the engines group their fp64 partial sums
differently, so a wrong choice shows).  The rule: the engines are tried in the order rows -> band -> split -> instance, a pinned
engine starts the walk at itself and lifts its own batch limit, and an un-grounded call on a single-pass frame that the row engine
does not take goes to the instance engine."""
import numpy as np
import pytest

from oracle import la3d_oracle as O

pytestmark = pytest.mark.gpu

# id, mask format, B, keyword arguments of the call, the engine the rule names
CASES = [
    ("u8-B8", "u8", 8, {}, "rows"),
    ("u8-B144", "u8", 144, {}, "rows"),
    ("u8-B256", "u8", 256, {}, "instance"),
    ("u8-ground-B1", "u8", 1, dict(ground=True), "band"),
    ("u8-ground-B64", "u8", 64, dict(ground=True), "band"),
    ("u8-ground-B144", "u8", 144, dict(ground=True), "band"),
    ("u8-ground-B192", "u8", 192, dict(ground=True), "instance"),
    ("u8-plain-B64", "u8", 64, dict(build="plain"), "band"),
    ("u8-sample-B64", "u8", 64, dict(sample=True), "instance"),
    ("u8-W600-B64", "u8", 64, dict(width=600), "instance"),
    ("rle-ground-B64", "rle", 64, dict(ground=True), "split"),
    ("rle-ground-B192", "rle", 192, dict(ground=True), "instance"),
    ("poly-ground-B64", "poly", 64, dict(ground=True), "split"),
    ("rle-B64", "rle", 64, {}, "instance"),
    ("rle-ground-filter-B64", "rle", 64, dict(ground=True, filter=True), "instance"),
    ("rle-ground-frame600-B64", "rle", 64, dict(ground=True, width=600), "instance"),
    ("pin-rows-u8-ground-B64", "u8", 64, dict(ground=True, pin="rows"), "band"),
    ("pin-band-rle-ground-B64", "rle", 64, dict(ground=True, pin="band"), "split"),
    ("pin-split-u8-sample-B64", "u8", 64, dict(sample=True, pin="split"), "instance"),
    ("pin-band-u8-ground-sample-B64", "u8", 64, dict(ground=True, sample=True, pin="band"), "instance"),
]


@pytest.fixture(scope="module")
def inputs():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bench

    dev = torch.device("cuda", 0)
    depth, masks, K, _, rects = bench.make_inputs(256, dev, 4321)
    ground = torch.as_tensor(np.array([[0.05, -0.97, 0.1, 1.2]] * 256) + 0.02 * np.random.RandomState(5).randn(256, 4), device=dev)
    return dev, depth, masks, K, rects, ground


def _fit(inputs, kind, B, kw, engine):
    """(boxes, status) of the call, pinned to `engine` (None: the library's choice)"""
    import torch

    import bench
    import labelany3d_amd as la

    dev, depth, masks, K, rects, ground = inputs
    W = kw.get("width", bench.W)
    d, m = depth[:B, :, :W].contiguous(), masks[:B, :, :W].contiguous()
    g = ground[:B] if kw.get("ground") else None
    si = None
    if kw.get("sample"):
        si = torch.as_tensor(la.draw_sample_idx(m.reshape(B, -1).sum(1), np.random.RandomState(B)), device=dev)
    engine = engine if engine is not None else kw.get("pin")
    if kind == "u8":
        f = la.InstanceFitter(B, bench.H, W, dev)
        boxes, status, _ = f.run(d, m, K, ground=g, sample_idx=si, engine=engine, build=kw.get("build"))
    else:
        if kind == "rle":
            src = dict(rles=[O.rle_encode(x) for x in m.cpu().numpy()])
        else:
            r0, c0, hh, ww = (a[:B] for a in rects)
            segs = [[[int(c), int(r), int(c + w - 1), int(r), int(c + w - 1), int(r + h - 1), int(c), int(r + h - 1)]]
                    for r, c, h, w in zip(r0, c0, hh, ww)]
            src = dict(polys=la.pack_polygons(segs, bench.H, W))
        with la.scheduling(engine=engine, build=kw.get("build")):
            out = la.fit_instances_ex(d, K, ground=g, sample_idx=si, filter=kw.get("filter"), device=dev, **src)
        boxes, status = out["boxes"], out["status"]
    torch.cuda.synchronize()
    return boxes.clone(), status.clone()


def _same(a, b):
    import torch

    return torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name,kind,B,kw,want", CASES, ids=[c[0] for c in CASES])
def test_dispatch_table(inputs, name, kind, B, kw, want):
    got = _fit(inputs, kind, B, kw, None)
    ref = _fit(inputs, kind, B, kw, want)
    assert _same(got, ref), f"{name}: not the records of the {want} engine"
    if want != "instance":
        inst = _fit(inputs, kind, B, kw, "instance")
        assert not _same(got, inst), f"{name}: the instance engine gives the same records, the table row proves nothing"
