"""Measured lines of the annotation bit-plane packers (include/la3d.h "annotations as bit planes"; RESULTS.md beside this file):
annotations -> instance point clouds through bit planes against the route a caller had before, alternated in ONE process so that the
spread of every line is known (the protocol of profiles/instance_points/bench_instance_points.py).

    python profiles/annotation_bits/bench_annotation_bits.py --out profiles/annotation_bits/bench_annotation_bits.json

Inputs: B = 1 / 16 / 256 / 1024 instances of 640 x 480 with config-2 masks (bench.make_inputs' rectangles of 8..300 x 8..330 px) as
COCO run lengths (one ones-run per column) and as polygons (the rectangle's four corners), three resident batches in rotation,
private depth planes; the annotation arrays are resident on the device.
  new.rle / new.poly   pack_rle_bits / pack_poly_bits, then instance_points on the MaskBits (capacity given: never synchronises)
  old.rle / old.poly   rle_decode / poly_decode, then instance_points on the boolean planes
  pack.rle / pack.poly the packer alone; ``model_MB`` = run or vertex bytes (counts + offsets | xy + ring_offsets + inst_rings) +
                       plane bytes (38 400 B per instance), ``model_GBps`` = that over the median time
Every line is warmed up, timed between two HIP events over ``steps`` calls, and the lines are alternated ``--reps`` times: first
the four route lines (new / old x rle / poly) among themselves, then the lines of the attribution (pack, decode, ip) among themselves.
``steps``: bench_instance_points.py's counts, raised until one run of a line lasts ``--min-ms`` (default 100 ms; from a pilot of
``steps`` calls): at small B a call is ~50 us of HOST time, and the host's time per call is not steady - the first ~100 calls of a
run are ~10 % slower and slower phases of some ms come and go (``fifths_host_us``: the mean host time per call of each fifth of
every run) -, so a run of 15 ms measures where its window fell, a run of 100 ms the line.
``not_slower_than_old``: the slowest run of the new route <= the fastest run of the old one.  ``host_us``: the same loop on the host's
clock (``time.perf_counter`` around the issue loop, no synchronisation inside): where it equals the event time the line is bound by
the Python wrappers, not by the GPU.  ``decode.*`` / ``ip.bits`` / ``ip.u8``: the parts of the two routes alone (the decoder; ``instance_points``
on resident planes), for that attribution.  The garbage collector is off inside a timed loop (``timeit``'s rule).  Prints one JSON document."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
p = argparse.ArgumentParser()
p.add_argument("--out", default=None)
p.add_argument("--reps", type=int, default=3)
p.add_argument("--batches", default="1,16,256,1024")
p.add_argument("--quick", action="store_true", help="a fifth of the steps (rehearsal)")
p.add_argument("--min-ms", type=float, default=100.0, help="a timed run lasts at least this long (0: the step table as it is)")
args = p.parse_args()
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import labelany3d_amd as la  # noqa: E402
from labelany3d_amd._lib import lib  # noqa: E402

H, W, R = bench.H, bench.W, 3
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()
STEPS = {1: 500, 16: 300, 256: 50, 1024: 20}   # (the new-route steps of bench_instance_points.py)


def rect_runs(rects):
    """config-2 rectangles -> (counts int32, offsets int64): column-major runs, zeros first - one ones-run of hh pixels per column"""
    r0, c0, hh, ww = (np.asarray(v, np.int64) for v in rects)
    counts, offsets = [], [0]
    for a, b, h, w in zip(r0, c0, hh, ww):
        c = np.empty(2 * w, np.int64)
        c[0::2] = H - h
        c[1::2] = h
        c[0] = b * H + a
        counts.append(c)
        offsets.append(offsets[-1] + len(c))
    return np.concatenate(counts).astype(np.int32), np.asarray(offsets, np.int64)


def rect_polys(rects):
    r0, c0, hh, ww = (np.asarray(v, np.int64) for v in rects)
    return la.pack_polygons([[[int(b), int(a), int(b + w - 1), int(a), int(b + w - 1), int(a + h - 1), int(b), int(a + h - 1)]]
                             for a, b, h, w in zip(r0, c0, hh, ww)], H, W)


def make_batches(B):
    out = []
    for r in range(R):
        depth, masks, K, npix, rects = bench.make_inputs(B, dev, 1234 + r)
        rects = tuple(np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in rects)
        counts, offsets = rect_runs(rects)
        xy, ro, ir, _, _ = rect_polys(rects)
        rle = (torch.as_tensor(counts, device=dev), torch.as_tensor(offsets, device=dev), H, W)
        poly = (torch.as_tensor(xy, device=dev), torch.as_tensor(ro, device=dev), torch.as_tensor(ir, device=dev), H, W)
        nwords = H * W // 32
        out.append(dict(depth=depth, mbool=masks.view(torch.bool), K=K, rows=int(npix), rle=rle, poly=poly,
                        rle_bytes=counts.nbytes + offsets.nbytes, poly_bytes=xy.nbytes + ro.nbytes + ir.nbytes,
                        planes=torch.empty((B, nwords), dtype=torch.int32, device=dev), area=torch.empty(B, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    return out


def pack(b, kind):
    fn = la.pack_rle_bits if kind == "rle" else la.pack_poly_bits
    return fn(b[kind], out=b["planes"], area=b["area"])


def new_route(b, kind):
    return la.instance_points(b["depth"], pack(b, kind), b["K"], capacity=b["rows"])


def old_route(b, kind):
    planes = la.rle_decode(b["rle"]) if kind == "rle" else la.poly_decode(b["poly"])
    return la.instance_points(b["depth"], planes, b["K"], capacity=b["rows"])


def time_line(fn, steps, warmup):
    for k in range(warmup):
        fn(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()   # (as timeit does: these lines are host-bound at small B, and a collection inside one run of a line is a stall of milliseconds)
    per = np.empty(steps)
    e0.record(st)
    t0 = tp = time.perf_counter()
    for k in range(steps):
        fn(warmup + k)
        tn = time.perf_counter()
        per[k], tp = tn - tp, tn
    e1.record(st)
    gc.enable()
    torch.cuda.synchronize()
    fifths = [float(c.mean() * 1e6) for c in np.array_split(per, 5)]
    return e0.elapsed_time(e1) * 1e3 / steps, (tp - t0) * 1e6 / steps, fifths   # us per call: HIP events, host issue loop, its fifths


def summarise(v):
    order = [t for t, _, _ in v]
    runs = sorted(order)
    return dict(median=float(np.median(runs)), min=runs[0], max=runs[-1], spread=runs[-1] - runs[0], runs=runs, in_order=order,
                host_us=float(np.median([h for _, h, _ in v])), fifths_host_us=[[round(x, 2) for x in f] for _, _, f in v])


result = dict(build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0), frame=[H, W], reps=args.reps, lines={})
for B in [int(x) for x in args.batches.split(",")]:
    batches = make_batches(B)
    steps = max(STEPS.get(B, 12) // (5 if args.quick else 1), 2)
    b0 = batches[0]
    for kind in ("rle", "poly"):   # the annotations ARE the config-2 masks, and the two routes give the same rows, bit for bit
        mb = pack(b0, kind)
        assert torch.equal(la.unpack_mask_bits(mb), b0["mbool"]), kind
        assert int(b0["area"].sum()) == b0["rows"]
        got, want = new_route(b0, kind), old_route(b0, kind)
        torch.cuda.synchronize()
        assert int(got.offsets[-1]) == b0["rows"] and int((got.status != 0).sum()) == 0
        assert torch.equal(torch.nan_to_num(got.points, nan=-7.0), torch.nan_to_num(want.points, nan=-7.0)), kind
        del got, want
    lines = {}
    for kind in ("rle", "poly"):
        lines[f"new.{kind}"] = lambda k, kd=kind: new_route(batches[k % R], kd)
        lines[f"old.{kind}"] = lambda k, kd=kind: old_route(batches[k % R], kd)
        lines[f"pack.{kind}"] = lambda k, kd=kind: pack(batches[k % R], kd)
        lines[f"decode.{kind}"] = lambda k, kd=kind: la.rle_decode(batches[k % R]["rle"]) if kd == "rle" else la.poly_decode(batches[k % R]["poly"])
    resident = [(pack(b, "rle"), la.rle_decode(b["rle"])) for b in batches]
    lines["ip.bits"] = lambda k: la.instance_points(batches[k % R]["depth"], resident[k % R][0], batches[k % R]["K"], capacity=batches[k % R]["rows"])
    lines["ip.u8"] = lambda k: la.instance_points(batches[k % R]["depth"], resident[k % R][1], batches[k % R]["K"], capacity=batches[k % R]["rows"])
    # a run lasts at least --min-ms: the steps of every line from a pilot of `steps` calls (not recorded)
    def pilot(fn):
        ev, host, _ = time_line(fn, steps, max(steps // 10, 1))
        return max(steps, int(np.ceil(args.min_ms * 1e3 / max(ev, host)))) if args.min_ms > 0 else steps
    nsteps = {name: pilot(fn) for name, fn in lines.items()}
    times = {k: [] for k in lines}
    # the four lines the requirement is about are alternated on their own, so that an alternation is as short as it can be (the host
    # changes speed by 5 - 13 % for seconds at a time, every line alike); the lines of the attribution follow, alternated likewise
    routes = [k for k in lines if k.startswith(("new.", "old."))]
    for group in (routes, [k for k in lines if k not in routes]):
        for _ in range(args.reps):
            for name in group:
                times[name].append(time_line(lines[name], nsteps[name], max(nsteps[name] // 10, 1)))
    res = {k: summarise(v) for k, v in times.items()}
    for kind in ("rle", "poly"):
        n, o, pk = res[f"new.{kind}"], res[f"old.{kind}"], res[f"pack.{kind}"]
        n["old_over_new"] = o["median"] / n["median"]
        n["not_slower_than_old"] = bool(n["max"] <= o["min"])
        mbytes = float(np.mean([b[f"{kind}_bytes"] for b in batches])) + B * (H * W // 8)
        pk.update(model_MB=mbytes / 1e6, model_GBps=mbytes / (pk["median"] * 1e-6) / 1e9)
    res["steps"] = nsteps
    res["rows"] = float(np.mean([b["rows"] for b in batches]))
    result["lines"][f"B={B}"] = res
    print(f"B={B}", {k: round(v["median"], 1) for k, v in res.items() if isinstance(v, dict) and "median" in v}, flush=True)
    del batches, b0, mb, resident, lines
    torch.cuda.empty_cache()

text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
