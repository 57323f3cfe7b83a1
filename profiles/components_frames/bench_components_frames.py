"""Measured lines of the frames form of connected components on bit planes (include/la3d.h "connected components on bit planes",
la3d_components_bits_frames; RESULTS.md beside this file): the resident ``FrameBits`` of a mixed-size shard -> the largest component
of every plane, or the planes without their islands, with the statistics in ONE call, against the route a caller had before - the
planes regrouped by size and one ``components_bits`` call per group -, alternated in ONE process so that the spread of every line is
known (the protocol of profiles/open_bits_frames/bench_open_bits_frames.py).

    python profiles/components_frames/bench_components_frames.py --out profiles/components_frames/bench_components_frames.json

Inputs: the project's mixed-size mix, as restated in profiles/open_bits_frames/bench_open_bits_frames.py: 256 images of the 18
``COCO_SIZES``, the share of a size falling off as 1 / rank, in a seeded arrival order; 1 instance per image (256 rows) and 7 (1792
rows, the full mix), each the union of three rectangles or ellipses XORed with 2 % salt noise; two sets in rotation.
  one.largest        largest_component_bits_frames(out =, return_stats = True): one kernel over every row
  one.drop           drop_islands_bits_frames(min_area = 16, out =, return_stats = True)
  one.stats          components_stats_frames(largest = True): the statistics-only call (out_bits = NULL)
  grouped.regroup    the parent's route, first half: the planes of each size gathered into a (B_g, words) tensor (one indexed copy per
                     size; the index tensors are built once, outside the clock)
  grouped.largest    second half: one largest_component_bits(out =, return_stats = True) per size on the gathered planes
  grouped.total      both halves (scattering the results back is not timed)
  grouped.drop       both halves with drop_islands_bits(min_area = 16)
Every line is warmed up and timed over ``steps`` calls between two HIP events with the host's clock beside them (``host_us``),
``steps`` raised until a run lasts ``--min-ms``, the lines alternated ``--reps`` times.  Before anything is timed the two routes are
compared bit for bit, planes and statistics.  Prints one JSON document."""
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
p.add_argument("--images", type=int, default=256)
p.add_argument("--per-image", default="1,7", help="instances per image, comma separated: one case each")
p.add_argument("--min-ms", type=float, default=60.0, help="a timed run lasts at least this long")
args = p.parse_args()
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import labelany3d_amd as la  # noqa: E402
from labelany3d_amd._lib import lib  # noqa: E402

COCO_SIZES = [(480, 640), (640, 480), (427, 640), (640, 427), (426, 640), (428, 640), (375, 500), (500, 375), (333, 500), (425, 640),
              (480, 480), (640, 640), (360, 640), (500, 333), (612, 612), (424, 640), (334, 500), (512, 640)]
R, MIN_AREA, MAX_RUNS = 2, 16, 16384
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()


def coco_mix(images, seed):
    """the sizes of ``images`` images: share 1 / rank over COCO_SIZES, in a seeded arrival order"""
    rs = np.random.RandomState(seed)
    share = 1.0 / np.arange(1, len(COCO_SIZES) + 1)
    share /= share.sum()
    n = np.maximum(1, np.round(share * images).astype(int))
    n[0] += images - n.sum()
    sizes = [s for s, k in zip(COCO_SIZES, n) for _ in range(k)]
    return [sizes[i] for i in rs.permutation(len(sizes))]


def make_stacks(sizes, per, seed):
    """one (per, h, w) uint8 stack per image, made on the device"""
    rs = np.random.RandomState(seed)
    gen = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for h, w in sizes:
        vv = torch.arange(h, device=dev)[:, None]
        uu = torch.arange(w, device=dev)[None, :]
        m = torch.zeros((per, h, w), dtype=torch.bool, device=dev)
        for j in range(per):
            for _ in range(3):
                cy, cx, hy, hx = rs.randint(0, h), rs.randint(0, w), rs.randint(8, h // 3), rs.randint(8, w // 3)
                if rs.rand() < 0.5:
                    m[j] |= ((vv - cy).abs() <= hy) & ((uu - cx).abs() <= hx)
                else:
                    m[j] |= ((vv - cy) / float(hy)) ** 2 + ((uu - cx) / float(hx)) ** 2 <= 1.0
        m ^= torch.rand((per, h, w), device=dev, generator=gen) < 0.02
        out.append(m.view(torch.uint8))
    return out


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


def summarise(v):
    runs = sorted(t for t, _ in v)
    return dict(median=float(np.median(runs)), min=runs[0], max=runs[-1], spread=runs[-1] - runs[0], in_order=[t for t, _ in v],
                host_us=float(np.median([h for _, h in v])))


sizes = coco_mix(args.images, 7)
result = dict(build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0), images=len(sizes),
              distinct_sizes=len(set(sizes)), min_area=MIN_AREA, max_runs=MAX_RUNS, reps=args.reps, lines={})
for per in (int(x) for x in args.per_image.split(",")):
    sets = []
    for r in range(R):
        pm = la.pack_mask_frames(make_stacks(sizes, per, 2300 + r))
        sets.append(dict(pm=pm, fb=la.pack_mask_bits_frames(pm)))
    pm = sets[0]["pm"]
    ii_h = sets[0]["fb"].image_index.cpu().numpy()
    offs_h = sets[0]["fb"].offsets.cpu().numpy()
    B = len(ii_h)
    # the groups of the parent's route: rows by size, the gather indices of their planes, their output buffers
    groups = []
    for h, w in sorted(set(sizes)):
        rows = np.flatnonzero(np.array([sizes[i] == (h, w) for i in ii_h]))
        wp = la.padded_width(w)
        words = h * wp // 32
        idx = torch.as_tensor(offs_h[rows][:, None] + np.arange(words)[None, :], device=dev)
        groups.append(dict(h=h, w=w, wp=wp, rows=rows, idx=idx, buf=torch.empty((len(rows), words), dtype=torch.int32, device=dev),
                           out=torch.empty((len(rows), words), dtype=torch.int32, device=dev)))
    out = torch.empty(sets[0]["fb"].bits.numel(), dtype=torch.int32, device=dev)

    def regroup(k):
        bits = sets[k % R]["fb"].bits
        for g in groups:
            torch.take(bits, g["idx"], out=g["buf"])

    def grouped_largest(k):
        return [la.largest_component_bits(la.MaskBits(g["buf"], g["h"], g["wp"], g["w"]), max_runs=MAX_RUNS, out=g["out"], return_stats=True)
                for g in groups]

    def grouped_total(k):
        regroup(k)
        return grouped_largest(k)

    def grouped_drop(k):
        regroup(k)
        return [la.drop_islands_bits(la.MaskBits(g["buf"], g["h"], g["wp"], g["w"]), MIN_AREA, max_runs=MAX_RUNS, out=g["out"], return_stats=True)
                for g in groups]

    def one_largest(k):
        d = sets[k % R]
        return la.largest_component_bits_frames(d["pm"], d["fb"], max_runs=MAX_RUNS, out=out, return_stats=True)

    def one_drop(k):
        d = sets[k % R]
        return la.drop_islands_bits_frames(d["pm"], d["fb"], MIN_AREA, max_runs=MAX_RUNS, out=out, return_stats=True)

    def one_stats(k):
        d = sets[k % R]
        return la.components_stats_frames(d["pm"], d["fb"], largest=True, max_runs=MAX_RUNS)

    # the routes give the same planes and statistics, bit for bit
    inputs = {}
    for tag, f_one, f_grouped in (("largest", one_largest, grouped_total), ("drop", one_drop, grouped_drop)):
        res, stats = f_one(0)
        per_group = f_grouped(0)
        o = res.offsets.cpu().numpy()
        kept = 0
        for g, (mb, st_g) in zip(groups, per_group):
            words = mb.bits.shape[1]
            got = torch.take(res.bits, torch.as_tensor(o[g["rows"]][:, None] + np.arange(words)[None, :], device=dev))
            assert torch.equal(got, mb.bits) and torch.equal(stats[torch.as_tensor(g["rows"], device=dev)], st_g), (tag, g["h"], g["w"])
            kept += int(st_g[:, 3].sum())
        sh = stats.cpu().numpy()
        assert kept > 0 and (sh[:, 0] > 0).all(), tag                        # every row labelled: none refused, none over capacity
        assert torch.equal(one_stats(0), stats) or tag != "largest"
        inputs = dict(components_median=float(np.median(sh[:, 0])), components_max=int(sh[:, 0].max()),
                      area_in_median=float(np.median(sh[:, 2])))
    lines = {
        "one.largest": one_largest,
        "one.drop": one_drop,
        "one.stats": one_stats,
        "grouped.regroup": regroup,
        "grouped.largest": grouped_largest,
        "grouped.total": grouped_total,
        "grouped.drop": grouped_drop,
    }
    nsteps = {}
    for name, fn in lines.items():   # a run lasts at least --min-ms: from a pilot
        ev, host = time_device(fn, 2, 1)
        nsteps[name] = max(2, int(np.ceil(args.min_ms * 1e3 / max(ev, host, 1e-3))))
    times = {k: [] for k in lines}
    for _ in range(args.reps):
        for name, fn in lines.items():
            times[name].append(time_device(fn, nsteps[name], max(nsteps[name] // 10, 1)))
    res = {k: summarise(v) for k, v in times.items()}
    for a, b in (("one.largest", "grouped.total"), ("one.drop", "grouped.drop")):
        res[a].update(grouped_over_one=res[b]["median"] / res[a]["median"],
                      slower_than_grouped_beyond_its_spread=bool(res[a]["median"] > res[b]["median"] + res[b]["spread"]))
    res["steps"] = nsteps
    res["rows"], res["groups"], res["inputs"] = B, len(groups), inputs
    result["lines"][f"rows={B}"] = res
    print(f"rows={B}", {k: round(v["median"], 1) for k, v in res.items() if isinstance(v, dict) and "median" in v}, flush=True)
    del sets, groups, out, pm
    torch.cuda.empty_cache()

text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
