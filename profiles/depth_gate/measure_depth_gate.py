"""Measured lines of the depth gate on bit planes (include/la3d.h "depth gate on bit planes"; RESULTS.md beside this file): resident
``MaskBits`` of 640 x 480 frames with the config-2 rectangles of bench.py and a private float32 depth plane per instance ->
``gate_depth_bits``, against the route a caller has today, against the floor - a pure pass over the same planes - and against the fit it
precedes, alternated in ONE process so that the spread of every line is known (the protocol of profiles/components/bench_components.py).

    python profiles/depth_gate/measure_depth_gate.py --out profiles/depth_gate/measure_depth_gate.json

Inputs: B = 1 / 16 / 256 / 1024 instances of bench.make_inputs (rectangles of 8 .. 300 x 8 .. 330 pixels, depth uniform in 0.5 .. 10),
three batches in rotation as bench.py rotates them.
  gate        gate_depth_bits(out =, return_stats = True): one kernel, planes and statistics, nothing leaves the device
  stats       depth_gate_stats: the statistics-only call (out_bits = NULL)
  gate.ties   gate_depth_bits on the same masks over a CONSTANT depth: every key ties, no bracket can be confirmed, both medians take the
              four radix rounds - what the fallback costs
  today       the route a caller has today (B <= --today-max): unpack_mask_bits, NaN-filled masked depth, two torch.nanmedian passes,
              compare, pack_mask_bits.  Its even-count rule differs (the lower middle value): a time baseline, not a parity one
  floor       bits_rects on the same planes: area and rectangle, a pure pass over the same bits
  fit         fit_instances_bits on the same planes and depth: the step the gate precedes
Every line is warmed up and timed over ``steps`` calls between two HIP events with the host's clock beside them (``host_us``), ``steps``
raised until a run lasts ``--min-ms``, the lines alternated ``--reps`` times.  Before anything is timed the gate is compared with the
NumPy restatement of the rule (tests/depth_gate_cases.py) on the first instances of the batch.
``fast_path``: the kernel does not say which selection path it took, so the verdict of its sample -> bracket -> count -> collect path is
re-enacted on the host for the first ``--enact`` instances of the batch, both medians, with the chunk list in ascending order (the
kernel's order depends on the order its atomics land in, so the sampled chunks - not the medians - may differ): the share of medians
whose bracket holds the middle ranks in bins of at most 6144 keys.  Prints one JSON document."""
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
p.add_argument("--today-max", type=int, default=256, help="largest batch the torch route is run at")
p.add_argument("--enact", type=int, default=32, help="instances whose selection path is re-enacted on the host")
args = p.parse_args()
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import labelany3d_amd as la  # noqa: E402
from labelany3d_amd._lib import lib  # noqa: E402
from tests import depth_gate_cases as DG  # noqa: E402

H, W, R = bench.H, bench.W, 3
CAP, SAMPLE = 6144, 2048          # RM_CAP and RM_SAMPLE of la3d_select.hpp
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()


def route_today(d, bits, out):
    B = d.shape[0]
    m = la.unpack_mask_bits(bits)
    x = torch.where(m, d, torch.full((), float("nan"), device=dev))
    med = torch.nanmedian(x.view(B, -1), dim=1).values
    dist = (x - med.view(B, 1, 1)).abs_()
    mad = torch.nanmedian(dist.view(B, -1), dim=1).values
    return la.pack_mask_bits(dist <= (4.5 * mad).view(B, 1, 1), out=out)


def keys(v):
    b = v.view(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def enact(values, chunk_of):
    """the verdict of the fast path for the float32 ``values`` of one mask (chunk_of: the 64-pixel chunk of each): "direct" (all keys
    fit the LDS buffer), "bracket" (confirmed), or the reason it falls back to the radix rounds"""
    n = len(values)
    if n <= CAP:
        return "direct"
    k = keys(values)
    cstep = (n + SAMPLE - 1) // SAMPLE
    active = np.unique(chunk_of)
    sample = np.sort(k[np.isin(chunk_of, active[::cstep])])[:CAP]
    ns = len(sample)
    if ns < 512:
        return "fallback:sample"
    w = ns // 12
    klo, khi = int(sample[ns // 2 - w]), int(sample[ns // 2 + w])
    width = khi - klo
    sh = 0 if width < 256 else width.bit_length() - 8
    rlo, rhi = (n // 2, n // 2) if n & 1 else (n // 2 - 1, n // 2)
    k64 = k.astype(np.int64)
    below = int((k64 < klo).sum())
    inside = k64[(k64 >= klo) & (k64 <= khi)]
    hist = np.bincount((inside - klo) >> sh, minlength=256)
    edges = below + np.concatenate([[0], np.cumsum(hist)])
    if rlo < below or rhi >= edges[-1]:
        return "fallback:bracket"
    b0, b1 = int(np.searchsorted(edges, rlo, "right")) - 1, int(np.searchsorted(edges, rhi, "right")) - 1
    return "bracket" if hist[b0:b1 + 1].sum() <= CAP else "fallback:bin"


def enact_batch(d, masks, levels, count):
    tally = {}
    chunk = (np.arange(H * W) // 64).reshape(H, W)
    for b in range(min(count, len(masks))):
        m = masks[b] & np.isfinite(d[b])
        for vals in (d[b][m], np.abs(d[b][m] - levels[b, 0])):
            verdict = enact(vals.astype(np.float32), chunk[m])
            tally[verdict] = tally.get(verdict, 0) + 1
    return tally


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


result = dict(build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0), frame=[H, W], reps=args.reps,
              unit="us per call", lines={})
for B in (int(x) for x in args.batches.split(",")):
    bs = []
    for r in range(R):
        depth, masks, K, n_masked, _ = bench.make_inputs(B, dev, 3000 + r)
        bs.append(dict(d=depth, bits=la.pack_mask_bits(masks), K=K, flat=torch.full((B, H, W), 2.25, device=dev),
                       out=torch.empty((B, H * W // 32), dtype=torch.int32, device=dev),
                       out_t=torch.empty((B, H * W // 32), dtype=torch.int32, device=dev), area=n_masked / B))
        if r == 0:
            masks0 = masks
        del masks
    b0 = bs[0]
    new, stats = la.gate_depth_bits(b0["d"], b0["bits"], return_stats=True)
    n = min(B, 4)                                     # the gate against the restatement, before anything is timed
    d_h, m_h = b0["d"][:max(n, min(B, args.enact))].cpu().numpy(), masks0[:max(n, min(B, args.enact))].cpu().numpy().astype(bool)
    keep, counts, levels = DG.gate_batch(d_h[:n], m_h[:n])
    assert np.array_equal(new.bits[:n].cpu().numpy().view(np.uint32), DG.pack(keep, W))
    assert np.array_equal(stats.counts[:n].cpu().numpy(), counts) and np.array_equal(stats.levels[:n].cpu().numpy(), levels, equal_nan=True)
    fast = enact_batch(d_h, m_h, stats.levels.cpu().numpy(), args.enact)
    del masks0
    lines = {
        "gate": lambda k: la.gate_depth_bits(bs[k % R]["d"], bs[k % R]["bits"], out=bs[k % R]["out"], return_stats=True),
        "stats": lambda k: la.depth_gate_stats(bs[k % R]["d"], bs[k % R]["bits"]),
        "gate.ties": lambda k: la.gate_depth_bits(bs[k % R]["flat"], bs[k % R]["bits"], out=bs[k % R]["out"], return_stats=True),
        "floor": lambda k: la.bits_rects(bs[k % R]["bits"]),
        "fit": lambda k: la.fit_instances_bits(bs[k % R]["d"], bs[k % R]["bits"], bs[k % R]["K"]),
    }
    if B <= args.today_max:
        lines["today"] = lambda k: route_today(bs[k % R]["d"], bs[k % R]["bits"], bs[k % R]["out_t"])
    nsteps = {}
    for name, fn in lines.items():                    # a run lasts at least --min-ms: from a pilot
        ev, host = time_device(fn, 2, 1)
        nsteps[name] = max(2, int(np.ceil(args.min_ms * 1e3 / max(ev, host, 1e-3))))
    times = {k: [] for k in lines}
    for _ in range(args.reps):
        for name, fn in lines.items():
            times[name].append(time_device(fn, nsteps[name], max(nsteps[name] // 10, 1)))
    res = {k: summarise(v) for k, v in times.items()}
    for k in ("gate", "stats", "gate.ties"):
        res[k]["over_floor"] = res[k]["median"] / res["floor"]["median"]
        res[k]["over_fit"] = res[k]["median"] / res["fit"]["median"]
        res[k]["us_per_plane"] = res[k]["median"] / B
    if "today" in res:
        res["today"]["over_gate"] = res["today"]["median"] / res["gate"]["median"]
    res["inputs"] = dict(mean_area=float(np.mean([b["area"] for b in bs])), kept_share=float(stats.counts[:, 2].sum() / max(int(stats.counts[:, 0].sum()), 1)))
    res["fast_path"] = dict(medians_enacted=int(sum(fast.values())), verdicts=fast)
    res["steps"] = nsteps
    result["lines"][str(B)] = res
    print(B, {k: round(v["median"], 1) for k, v in res.items() if isinstance(v, dict) and "median" in v}, fast, file=sys.stderr, flush=True)
    del bs, b0, new, stats
    torch.cuda.empty_cache()

doc = json.dumps(result, indent=1)
if args.out:
    with open(args.out, "w") as f:
        f.write(doc + "\n")
print(doc)
