"""Measured lines of the run-length encoder of bit planes (include/la3d.h "bit planes as run lengths"; RESULTS.md beside this file):
resident ``MaskBits`` -> ``RleRuns`` on the device against the only route the parent commit offers - unpack to u8, copy to the host,
encode with NumPy, upload the counts -, alternated in ONE process so that the spread of every line is known.

    python profiles/rle_encode/measure_rle_encode.py --out profiles/rle_encode/measure_rle_encode.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/rle_encode/measure_rle_encode.py --kernels-only 1024   # a run of its own

Inputs: B = 1 / 16 / 256 / 1024 instances of 640 x 480, resident as bit planes (38 400 B each), two mask sets:
  rect   config-2 rectangles (bench.make_inputs: 8..300 x 8..330 px): two runs per covered column
  blob   the union of two random ellipses (radii 25..110 px): a few hundred runs per instance
Lines (every call ends in a host synchronisation of its own, so the time between the two HIP events around ``steps`` calls is the
time of the calls):
  new        rle_encode_bits(mb): two stages + the one read-back of offsets[-1] that sizes ``counts``
  new.cap    rle_encode_bits(mb, capacity=known total): the same chain without the read-back, one synchronise per call added here
  old        unpack_mask_bits(mb) -> .cpu() (307 200 B per instance) -> NumPy encoder per mask -> counts and offsets uploaded
``bytes``: what each route moves by its own arithmetic - new: the planes read by both stages, the workspace written and read, runs,
offsets and counts written; old: the planes read, the u8 planes written, copied to the host, the counts copied back.
Before the timing the script checks that both routes give the same lists.  Prints one JSON document."""
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
p.add_argument("--kernels-only", type=int, default=0, help="B: 20 calls of the new route on each mask set and nothing else (for rocprofv3)")
args = p.parse_args()
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import labelany3d_amd as la  # noqa: E402
from labelany3d_amd._lib import lib  # noqa: E402

H, W = bench.H, bench.W
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
NEW_STEPS = {1: 400, 16: 400, 256: 100, 1024: 40}
OLD_STEPS = {1: 40, 16: 8, 256: 2, 1024: 1}


def blobs(B, seed):
    """(B, H, W) bool on the device: the union of two random ellipses per instance"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = torch.rand((B, 2, 4), generator=g).to(dev)
    vv = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    uu = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    out = torch.zeros((B, H, W), dtype=torch.bool, device=dev)
    for k in range(2):
        cy, cx = 110 + r[:, k, 0] * (H - 220), 110 + r[:, k, 1] * (W - 220)
        ry, rx = 25 + r[:, k, 2] * 85, 25 + r[:, k, 3] * 85
        out |= ((vv - cy[:, None, None]) / ry[:, None, None]) ** 2 + ((uu - cx[:, None, None]) / rx[:, None, None]) ** 2 < 1.0
    return out


def numpy_encode(mask):
    """binary_mask_to_rle (reference src/download_coconut.py:167-175) on one (H, W) u8 / bool plane: column-major runs, zeros first"""
    flat = np.asarray(mask).ravel(order="F") != 0
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate([[0], change, [flat.size]]))
    return np.concatenate([[0], counts]) if flat[0] else counts


def old_route(mb):
    planes = la.unpack_mask_bits(mb).cpu().numpy()
    parts = [numpy_encode(m) for m in planes]
    offsets = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(c) for c in parts], out=offsets[1:])
    counts = np.concatenate(parts).astype(np.int32)
    out = la.RleRuns(torch.as_tensor(counts, device=dev), torch.as_tensor(offsets, device=dev), mb.H, mb.frame_width)
    torch.cuda.synchronize()
    return out


def time_line(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    gc.disable()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    gc.enable()
    return e0.elapsed_time(e1) * 1e3 / steps, (t1 - t0) * 1e6 / steps


def mask_sets(B):
    _, masks, _, _, _ = bench.make_inputs(B, dev, 1234)
    return {"rect": la.pack_mask_bits(masks.view(torch.bool)), "blob": la.pack_mask_bits(blobs(B, 77))}


if args.kernels_only:
    for name, mb in mask_sets(args.kernels_only).items():
        for _ in range(20):
            la.rle_encode_bits(mb)
    torch.cuda.synchronize()
    sys.exit(0)

doc = {"device": torch.cuda.get_device_name(0), "build_info": lib.la3d_build_info().decode(), "H": H, "W": W, "reps": args.reps, "lines": []}
for B in (int(b) for b in args.batches.split(",")):
    for name, mb in mask_sets(B).items():
        new, old = la.rle_encode_bits(mb), old_route(mb)
        assert torch.equal(new.counts, old.counts) and torch.equal(new.offsets, old.offsets), (B, name)
        total = int(new.offsets[-1])
        lines = {"new": lambda: la.rle_encode_bits(mb),
                 "new.cap": lambda: (la.rle_encode_bits(mb, capacity=total), torch.cuda.synchronize()),
                 "old": lambda: old_route(mb)}
        runs = {k: [] for k in lines}
        for rep in range(args.reps):   # alternated: new, new.cap, old, new, new.cap, old, ...
            for k, fn in lines.items():
                steps = OLD_STEPS[B] if k == "old" else NEW_STEPS[B]
                runs[k].append(time_line(fn, steps, max(steps // 10, 1)))
        plane, ws = H * W // 8, W * 8
        model = {"new": B * (2 * plane + 2 * ws + 4 + 8) + 4 * total, "old": B * (plane + 2 * H * W) + 4 * total + 8 * (B + 1)}
        rec = {"B": B, "masks": name, "runs_total": total, "runs_per_instance": total / B, "bytes": model}
        for k, v in runs.items():
            ev = sorted(x[0] for x in v)
            rec[k] = {"event_us": [round(x[0], 2) for x in v], "host_us": [round(x[1], 2) for x in v], "median_us": round(ev[len(ev) // 2], 2),
                      "min_us": round(ev[0], 2), "max_us": round(ev[-1], 2), "steps": OLD_STEPS[B] if k == "old" else NEW_STEPS[B]}
        rec["old_over_new"] = round(rec["old"]["median_us"] / rec["new"]["median_us"], 1)
        doc["lines"].append(rec)
        print(f"| {B} | {name} | {total / B:.0f} | {rec['new']['median_us']} [{rec['new']['min_us']} .. {rec['new']['max_us']}] | "
              f"{rec['new.cap']['median_us']} [{rec['new.cap']['min_us']} .. {rec['new.cap']['max_us']}] | "
              f"{rec['old']['median_us']} [{rec['old']['min_us']} .. {rec['old']['max_us']}] | {rec['old_over_new']} | "
              f"{model['new'] / 1e6:.2f} | {model['old'] / 1e6:.2f} |", file=sys.stderr, flush=True)
        del mb, new, old
        torch.cuda.empty_cache()
text = json.dumps(doc, indent=1)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
print(text)
