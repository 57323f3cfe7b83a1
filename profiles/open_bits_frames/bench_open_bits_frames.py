"""Measured lines of the frames form of the opening on bit planes (include/la3d.h "morphology on bit planes", la3d_open_bits_frames;
RESULTS.md beside this file): the resident ``FrameBits`` of a mixed-size shard -> the opened planes with their areas and rectangles
in ONE call, against the route a caller had before - the planes regrouped by size and one ``open_bits`` call per group -, alternated
in ONE process so that the spread of every line is known (the protocol of profiles/open_bits/bench_open_bits.py).

    python profiles/open_bits_frames/bench_open_bits_frames.py --out profiles/open_bits_frames/bench_open_bits_frames.json

Inputs: the project's mixed-size mix (profiles/frames_bits/measure_frames_bits.py, restated here because that script runs on import):
256 images of the 18 ``COCO_SIZES``, the share of a size falling off as 1 / rank, in a seeded arrival order; 1 instance per image (256
rows) and 7 (1792 rows, the full mix), each the union of three rectangles or ellipses XORed with 2 % salt noise; two sets in rotation.
  one.x4          open_bits_frames(k = 7, upscale = 4, image_index = host copy, out =, return_stats = True): the compact layout; the
                  offsets go up in one copy per call
  one.x4.stride   the same with image_index = None: nothing uploaded, the planes a uniform stride apart
  one.x1          one.x4 at upscale = 1
  grouped.regroup the parent's route, first half: the planes of each size gathered into a (B_g, words) tensor (one indexed copy per
                  size; the index tensors are built once, outside the clock)
  grouped.open    second half: one open_bits(k = 7, upscale = 4, out =, return_stats = True) per size on the gathered planes
  grouped.total   both halves
  grouped.x1      grouped.total at upscale = 1
Every line is warmed up and timed over ``steps`` calls between two HIP events with the host's clock beside them (``host_us``),
``steps`` raised until a run lasts ``--min-ms``, the lines alternated ``--reps`` times.  Before anything is timed the two routes are
compared bit for bit.  Prints one JSON document."""
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
K, R = 7, 2
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
              distinct_sizes=len(set(sizes)), k=K, reps=args.reps, lines={})
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
        groups.append(dict(h=h, w=w, wp=wp, rows=rows, idx=idx, buf=torch.empty((len(rows), words), dtype=torch.int32, device=dev)))
    outs = {}
    for s in (1, 4):
        total = la.frame_bits_offsets(la.scaled_frames(pm, s, device="cpu").table_host, ii_h)[1]
        gh, gw = la.scaled_frames(pm, s, device="cpu").H, la.scaled_frames(pm, s, device="cpu").W
        outs[s] = dict(compact=torch.empty(total, dtype=torch.int32, device=dev),
                       stride=torch.empty(B * ((gh * gw // 32 + 3) // 4 * 4), dtype=torch.int32, device=dev) if s == 4 else None,
                       grouped=[torch.empty((len(g["rows"]), s * g["h"] * la.padded_width(s * g["w"]) // 32), dtype=torch.int32, device=dev)
                                for g in groups])

    def regroup(k):
        bits = sets[k % R]["fb"].bits
        for g in groups:
            torch.take(bits, g["idx"], out=g["buf"])

    def grouped_open(k, s=4):
        return [la.open_bits(la.MaskBits(g["buf"], g["h"], g["wp"], g["w"]), k=K, upscale=s, out=o, return_stats=True)
                for g, o in zip(groups, outs[s]["grouped"])]

    def grouped_total(k, s=4):
        regroup(k)
        return grouped_open(k, s)

    def one(k, s=4, index=ii_h, layout="compact"):
        d = sets[k % R]
        return la.open_bits_frames(d["pm"], d["fb"], k=K, upscale=s, image_index=index, out=outs[s][layout], return_stats=True)

    # the routes give the same planes and statistics, bit for bit
    for s in (1, 4):
        res, stats = one(0, s)
        per_group = grouped_total(0, s)
        o = res.offsets.cpu().numpy()
        any_set = 0
        for g, (mb, st_g) in zip(groups, per_group):
            words = mb.bits.shape[1]
            got = torch.take(res.bits, torch.as_tensor(o[g["rows"]][:, None] + np.arange(words)[None, :], device=dev))
            assert torch.equal(got, mb.bits) and torch.equal(stats[torch.as_tensor(g["rows"], device=dev)], st_g), (s, g["h"], g["w"])
            any_set += int(st_g[:, 0].sum())
        assert any_set > 0
    lines = {
        "one.x4": lambda k: one(k),
        "one.x4.stride": lambda k: one(k, 4, None, "stride"),
        "one.x1": lambda k: one(k, 1),
        "grouped.regroup": regroup,
        "grouped.open": grouped_open,
        "grouped.total": grouped_total,
        "grouped.x1": lambda k: grouped_total(k, 1),
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
    res["one.x4"].update(grouped_over_one=res["grouped.total"]["median"] / res["one.x4"]["median"],
                         slower_than_grouped_beyond_its_spread=bool(res["one.x4"]["median"] > res["grouped.total"]["median"] + res["grouped.total"]["spread"]))
    res["one.x1"].update(grouped_over_one=res["grouped.x1"]["median"] / res["one.x1"]["median"],
                         slower_than_grouped_beyond_its_spread=bool(res["one.x1"]["median"] > res["grouped.x1"]["median"] + res["grouped.x1"]["spread"]))
    res["steps"] = nsteps
    res["rows"], res["groups"] = B, len(groups)
    result["lines"][f"rows={B}"] = res
    print(f"rows={B}", {k: round(v["median"], 1) for k, v in res.items() if isinstance(v, dict) and "median" in v}, flush=True)
    del sets, groups, outs, pm
    torch.cuda.empty_cache()

text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
