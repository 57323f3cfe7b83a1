"""Measured lines of connected components on bit planes (include/la3d.h "connected components on bit planes"; RESULTS.md beside this
file): resident ``MaskBits`` of 640 x 480 frames -> the largest component, or the plane without its islands, with the statistics,
against the host route it replaces and against the floor - a pure pass over the same planes -, alternated in ONE process so that the
spread of every line is known (the protocol of profiles/open_bits/bench_open_bits.py).

    python profiles/components/bench_components.py --out profiles/components/bench_components.json

Inputs: B = 1 / 16 / 256 / 1024 planes, each the union of three rectangles or ellipses XORed with 2 % salt noise; three batches in
rotation.  The run count and the component count of the inputs are reported (``inputs``).
  largest        largest_component_bits(out =, return_stats = True): one kernel, planes and statistics, nothing leaves the device
  drop           drop_islands_bits(min_area = 16, out =, return_stats = True)
  largest.mr8192 largest with max_runs = 8192: half the LDS per workgroup (32 KiB instead of 64), twice the workgroups per CU
  stats          components_stats(largest = True): the statistics-only call (out_bits = NULL)
  floor          bits_rects of the parent commit on the same planes: area and rectangle, a pure pass over the same bytes
  host           the host route (B <= 16 only): unpack_mask_bits, device-to-host copy, scipy.ndimage.label, np.bincount, keep the
                 largest, pack_mask_bits of the result (host clock, ends synchronised)
Every line is warmed up and timed over ``steps`` calls - device lines between two HIP events with the host's clock beside them
(``host_us``), host lines on the host's clock around a loop that ends in a synchronise -, ``steps`` raised until a run lasts
``--min-ms``, the lines alternated ``--reps`` times.  Before anything is timed the routes are compared bit for bit.  Prints one JSON
document."""
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
p.add_argument("--min-ms", type=float, default=60.0, help="a timed run lasts at least this long")
p.add_argument("--host-max", type=int, default=16, help="largest batch the host route is run at")
args = p.parse_args()
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import labelany3d_amd as la  # noqa: E402
from labelany3d_amd._lib import lib  # noqa: E402

H, W, R, MIN_AREA = 480, 640, 3, 16
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()


def make_batch(B, seed):
    """B planes: 32 seeded shapes in rotation, each plane with salt noise of its own"""
    rs = np.random.RandomState(seed)
    vv, uu = np.mgrid[0:H, 0:W]
    shapes = np.zeros((min(B, 32), H, W), bool)
    for b in range(len(shapes)):
        for _ in range(3):
            cy, cx, hy, hx = rs.randint(0, H), rs.randint(0, W), rs.randint(8, H // 3), rs.randint(8, W // 3)
            if rs.rand() < 0.5:
                shapes[b] |= (np.abs(vv - cy) <= hy) & (np.abs(uu - cx) <= hx)
            else:
                shapes[b] |= ((vv - cy) / float(hy)) ** 2 + ((uu - cx) / float(hx)) ** 2 <= 1.0
    noise = torch.rand((B, H, W), generator=torch.Generator().manual_seed(seed)) < 0.02
    return shapes[np.arange(B) % len(shapes)] ^ noise.numpy()


def route_host(bits, out):
    from scipy import ndimage

    m = la.unpack_mask_bits(bits).cpu().numpy()
    keep = np.zeros_like(m)
    for b, one in enumerate(m):
        labels, n = ndimage.label(one, np.ones((3, 3), int))
        if n:
            keep[b] = labels == 1 + int(np.argmax(np.bincount(labels.reshape(-1))[1:]))
    return la.pack_mask_bits(torch.as_tensor(keep.view(np.uint8), device=dev), out=out)


def time_device(fn, steps, warmup):
    for k in range(warmup):
        fn(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    e0.record(st)
    t0 = time.perf_counter()
    for k in range(steps):
        fn(warmup + k)
    t1 = time.perf_counter()
    e1.record(st)
    gc.enable()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps, (t1 - t0) * 1e6 / steps


def time_host(fn, steps, warmup):
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    t0 = time.perf_counter()
    for k in range(steps):
        fn(warmup + k)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    gc.enable()
    us = (t1 - t0) * 1e6 / steps
    return us, us


def summarise(v):
    runs = sorted(t for t, _ in v)
    return dict(median=float(np.median(runs)), min=runs[0], max=runs[-1], spread=runs[-1] - runs[0], in_order=[t for t, _ in v],
                host_us=float(np.median([h for _, h in v])))


result = dict(build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0), frame=[H, W], min_area=MIN_AREA, reps=args.reps,
              unit="us per call", lines={})
for B in (int(x) for x in args.batches.split(",")):
    bs = []
    for r in range(R):
        u8 = torch.as_tensor(make_batch(B, 2000 + r).view(np.uint8), device=dev)
        bs.append(dict(bits=la.pack_mask_bits(u8), out=torch.empty((B, H * W // 32), dtype=torch.int32, device=dev),
                       out_h=torch.empty((B, H * W // 32), dtype=torch.int32, device=dev)))
        del u8
    b0 = bs[0]
    full = la.components_stats(b0["bits"]).cpu().numpy()
    assert (full[:, 0] > 0).all()                     # no plane is beyond max_runs
    probe = la.components_stats(b0["bits"], max_runs=1).cpu().numpy()
    inputs = dict(runs_median=float(np.median(probe[:, 1])), runs_max=int(probe[:, 1].max()), components_median=float(np.median(full[:, 0])),
                  components_max=int(full[:, 0].max()))
    new, new_stats = la.largest_component_bits(b0["bits"], return_stats=True)
    assert torch.equal(la.bits_rects(new), new_stats[:, 3:])
    if B <= args.host_max:                            # the routes give the same planes, bit for bit
        assert torch.equal(route_host(b0["bits"], b0["out_h"]).bits, new.bits)
    lines = {
        "largest": (lambda k: la.largest_component_bits(bs[k % R]["bits"], out=bs[k % R]["out"], return_stats=True), time_device),
        "drop": (lambda k: la.drop_islands_bits(bs[k % R]["bits"], MIN_AREA, out=bs[k % R]["out"], return_stats=True), time_device),
        "largest.mr8192": (lambda k: la.largest_component_bits(bs[k % R]["bits"], out=bs[k % R]["out"], return_stats=True, max_runs=8192), time_device),
        "stats": (lambda k: la.components_stats(bs[k % R]["bits"], largest=True), time_device),
        "floor": (lambda k: la.bits_rects(bs[k % R]["bits"]), time_device),
    }
    if B <= args.host_max:
        lines["host"] = (lambda k: route_host(bs[k % R]["bits"], bs[k % R]["out_h"]), time_host)
    nsteps = {}
    for name, (fn, timer) in lines.items():           # a run lasts at least --min-ms: from a pilot
        ev, host = timer(fn, 2, 1)
        nsteps[name] = max(2, int(np.ceil(args.min_ms * 1e3 / max(ev, host, 1e-3))))
    times = {k: [] for k in lines}
    for _ in range(args.reps):
        for name, (fn, timer) in lines.items():
            times[name].append(timer(fn, nsteps[name], max(nsteps[name] // 10, 1)))
    res = {k: summarise(v) for k, v in times.items()}
    for k in ("largest", "drop", "largest.mr8192", "stats"):
        res[k]["over_floor"] = res[k]["median"] / res["floor"]["median"]
        res[k]["us_per_plane"] = res[k]["median"] / B
    if "host" in res:
        res["host"]["over_largest"] = res["host"]["median"] / res["largest"]["median"]
    res["inputs"] = inputs
    res["steps"] = nsteps
    result["lines"][str(B)] = res
    print(B, {k: round(v["median"], 1) for k, v in res.items() if isinstance(v, dict) and "median" in v}, inputs, file=sys.stderr, flush=True)
    del bs
    torch.cuda.empty_cache()

doc = json.dumps(result, indent=1)
if args.out:
    with open(args.out, "w") as f:
        f.write(doc + "\n")
print(doc)
