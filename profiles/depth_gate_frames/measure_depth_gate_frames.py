"""Measured lines of the frames form of the depth gate on bit planes (include/la3d.h "depth gate on bit planes",
la3d_depth_gate_bits_frames; RESULTS.md beside this file): the resident ``FrameBits`` of a mixed-size shard and the depth of its images,
as it is stored, -> the gated planes and their statistics in ONE call, against the routes a caller had before, alternated in ONE
process so that the spread of every line is known (the protocol of profiles/components_frames/bench_components_frames.py).

    python profiles/depth_gate_frames/measure_depth_gate_frames.py --out profiles/depth_gate_frames/measure_depth_gate_frames.json

Inputs: the project's mixed-size mix, as restated in profiles/components_frames/bench_components_frames.py: 256 images of the 18
``COCO_SIZES``, the share of a size falling off as 1 / rank, in a seeded arrival order; 1 instance per image (256 rows) and 7 (1792
rows, the full mix), each the union of three rectangles or ellipses XORed with 2 % salt noise; per image a tilted depth plane of 2 - 9 m
with 5 cm noise and 1 % pixels of the depth stage's fill value (10000.0); two sets in rotation.
  one.gate           gate_depth_bits_frames(out =, return_stats = True) on the float32 PackedFrames: one kernel over every row
  one.stats          depth_gate_stats_frames: the statistics-only call (out_bits = NULL)
  grouped.gate       the route callers had: one gate_depth_bits(image_index =, out =, return_stats = True) per size, on planes and depth
                     planes that are ALREADY regrouped by size and resident - the regrouping is not in this line
  grouped.regroup    what that route pays before it: the planes of each size gathered into a (B_g, words) tensor and the depth planes of
                     each size into a (P_g, H, pitch) tensor (one indexed copy each per size; the index tensors are built once, outside
                     the clock); scattering the gated planes back is not timed at all
  f16.one / u16.one  gate_depth_bits_frames on the float16 / uint16 (millimetres, zero is a hole) PackedFrames16 of the same depth
  f16.unpack+f32 / u16.unpack+f32   unpack_depth16 of the whole 16-bit buffer to float32, then the float32 frames call
Every line is warmed up and timed over ``steps`` calls between two HIP events with the host's clock beside them (``host_us``),
``steps`` raised until a run lasts ``--min-ms``, the lines alternated ``--reps`` times.  Before anything is timed the routes are
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
R, SCALE = 2, 0.001
if not torch.cuda.is_available():
    raise SystemExit("this measurement needs the GPU: nothing is timed without one")
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


def make_depth(sizes, seed):
    """one float32 (h, w) map per image, made on the device: a tilted plane of 2 - 9 m, 5 cm noise, 1 % fill values"""
    rs = np.random.RandomState(seed)
    gen = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for h, w in sizes:
        vv = torch.arange(h, device=dev, dtype=torch.float32)[:, None]
        uu = torch.arange(w, device=dev, dtype=torch.float32)[None, :]
        d = 2.0 + 3.0 * rs.rand() + 0.004 * uu + 0.006 * vv + 0.05 * torch.randn((h, w), device=dev, generator=gen)
        d[torch.rand((h, w), device=dev, generator=gen) < 0.01] = 10000.0
        out.append(d.contiguous())
    return out


def as_u16(d):   # millimetres: rint, clamped to the range (the rule of la3d_pack_depth16), as the bit patterns of uint16
    return torch.clamp(torch.round(d / SCALE), 0, 65535).to(torch.int32).to(torch.int16).view(torch.uint16)


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


def unpacked(pf16):
    flat = la.unpack_depth16(la.Depth16(pf16.data.view(1, -1), pf16.scale, pf16.zero_is_hole)).view(-1)
    return la.PackedFrames(flat, pf16.table, pf16.table_host, pf16.H, pf16.W, pf16.sizes)


sizes = coco_mix(args.images, 7)
result = dict(build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0), images=len(sizes),
              distinct_sizes=len(set(sizes)), reps=args.reps, u16_scale=SCALE, lines={})
depth_sets = []
for r in range(R):
    maps = make_depth(sizes, 4100 + r)
    depth_sets.append(dict(f32=la.pack_frames(maps), f16=la.pack_frames([m.half() for m in maps], dtype="f16"),
                           u16=la.pack_frames([as_u16(m) for m in maps], dtype="u16", scale=SCALE, zero_is_hole=True)))
    del maps
table = depth_sets[0]["f32"].table_host
result["bounds"] = dict(H=depth_sets[0]["f32"].H, W=depth_sets[0]["f32"].W)
for per in (int(x) for x in args.per_image.split(",")):
    sets = []
    for r in range(R):
        pm = la.pack_mask_frames(make_stacks(sizes, per, 2300 + r))
        sets.append(dict(fb=la.pack_mask_bits_frames(pm), **depth_sets[r]))
        del pm
    ii_h = sets[0]["fb"].image_index.cpu().numpy()
    offs_h = sets[0]["fb"].offsets.cpu().numpy()
    B = len(ii_h)
    # the groups of the route callers had: rows by size, the gather indices of their planes and of their images' depth planes
    groups = []
    for h, w in sorted(set(sizes)):
        rows = np.flatnonzero(np.array([sizes[i] == (h, w) for i in ii_h]))
        imgs = np.flatnonzero(np.array([s == (h, w) for s in sizes]))
        local = {int(q): j for j, q in enumerate(imgs)}
        wp = la.padded_width(w)
        words = h * wp // 32
        idx = torch.as_tensor(offs_h[rows][:, None] + np.arange(words)[None, :], device=dev)
        didx = torch.as_tensor(table["depth_offset"][imgs][:, None] + np.arange(h * wp)[None, :], device=dev)
        groups.append(dict(h=h, w=w, wp=wp, rows=rows, idx=idx, didx=didx,
                           ii=torch.as_tensor(np.array([local[int(ii_h[n])] for n in rows], np.int32), device=dev),
                           buf=[torch.empty((len(rows), words), dtype=torch.int32, device=dev) for _ in range(R)],
                           dep=[torch.empty((len(imgs), h, wp), dtype=torch.float32, device=dev) for _ in range(R)],
                           out=torch.empty((len(rows), words), dtype=torch.int32, device=dev)))
    out = torch.empty(sets[0]["fb"].bits.numel(), dtype=torch.int32, device=dev)

    def regroup(k):
        d = sets[k % R]
        for g in groups:
            torch.take(d["fb"].bits, g["idx"], out=g["buf"][k % R])
            torch.take(d["f32"].depth, g["didx"], out=g["dep"][k % R].view(len(g["didx"]), -1))

    def grouped_gate(k):   # (the regrouped inputs of set k % R are resident: regroup(0), regroup(1) ran before the clock)
        return [la.gate_depth_bits(g["dep"][k % R], la.MaskBits(g["buf"][k % R], g["h"], g["wp"], g["w"]), image_index=g["ii"], out=g["out"],
                                   return_stats=True) for g in groups]

    def one(kind):
        def fn(k):
            d = sets[k % R]
            return la.gate_depth_bits_frames(d[kind], d["fb"], out=out, return_stats=True)
        return fn

    def one_stats(k):
        d = sets[k % R]
        return la.depth_gate_stats_frames(d["f32"], d["fb"])

    def via_unpack(kind):
        def fn(k):
            d = sets[k % R]
            return la.gate_depth_bits_frames(unpacked(d[kind]), d["fb"], out=out, return_stats=True)
        return fn

    for r in range(R):
        regroup(r)
    torch.cuda.synchronize()
    # the routes give the same planes and statistics, bit for bit
    res, stats = one("f32")(0)
    o = res.offsets.cpu().numpy()
    for g, (mb, st_g) in zip(groups, grouped_gate(0)):
        words = mb.bits.shape[1]
        rows_d = torch.as_tensor(g["rows"], device=dev)
        got = torch.take(res.bits, torch.as_tensor(o[g["rows"]][:, None] + np.arange(words)[None, :], device=dev))
        assert torch.equal(got, mb.bits) and torch.equal(stats.counts[rows_d], st_g.counts), (g["h"], g["w"])
        assert torch.equal(stats.levels[rows_d].view(torch.int32), st_g.levels.view(torch.int32)), (g["h"], g["w"])
    sh = stats.counts.cpu().numpy()
    assert (sh[:, 0] > 0).all() and (sh[:, 2] < sh[:, 1]).any()          # no row refused; the gate drops pixels (the fill is finite: all valid)
    assert torch.equal(one_stats(0).counts, stats.counts)
    for kind in ("f16", "u16"):
        a, sa = one(kind)(0)
        planes_a, counts_a, levels_a = a.bits.clone(), sa.counts.clone(), sa.levels.clone()
        b, sb = via_unpack(kind)(0)
        sel = torch.as_tensor(np.concatenate([offs_h[n] + np.arange(int(table["H"][ii_h[n]]) * int(table["W"][ii_h[n]]) // 32) for n in range(B)]),
                              device=dev)
        assert torch.equal(torch.take(planes_a, sel), torch.take(b.bits, sel)) and torch.equal(counts_a, sb.counts), kind
        assert torch.equal(levels_a.view(torch.int32), sb.levels.view(torch.int32)), kind
        del sel
    inputs = dict(area_in_median=float(np.median(sh[:, 0])), n_valid_median=float(np.median(sh[:, 1])), area_out_median=float(np.median(sh[:, 2])))
    lines = {
        "one.gate": one("f32"),
        "one.stats": one_stats,
        "grouped.gate": grouped_gate,
        "grouped.regroup": regroup,
        "f16.one": one("f16"),
        "f16.unpack+f32": via_unpack("f16"),
        "u16.one": one("u16"),
        "u16.unpack+f32": via_unpack("u16"),
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
    for a, b in (("one.gate", "grouped.gate"), ("f16.one", "f16.unpack+f32"), ("u16.one", "u16.unpack+f32"), ("f16.one", "one.gate"),
                 ("u16.one", "one.gate")):
        res[a][f"{b}_over_this"] = res[b]["median"] / res[a]["median"]
        res[a][f"slower_than_{b}_beyond_its_spread"] = bool(res[a]["median"] > res[b]["median"] + res[b]["spread"])
    res["steps"] = nsteps
    res["rows"], res["groups"], res["inputs"] = B, len(groups), inputs
    result["lines"][f"rows={B}"] = res
    print(f"rows={B}", {k: round(v["median"], 1) for k, v in res.items() if isinstance(v, dict) and "median" in v}, flush=True)
    del sets, groups, out
    torch.cuda.empty_cache()

text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
