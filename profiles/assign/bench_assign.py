"""Measured lines of the assignment on the device (include/la3d.h "assignment on the device"; RESULTS.md beside this file): resident
``MaskBits`` of 640 x 480 -> the per-image mask IoU and the assignment that reads it, and the box form of ``combine``'s pass 3,
against the route a caller had before - the matrix copied to the host, ``scipy.optimize.linear_sum_assignment`` per group, the result
uploaded -, alternated in ONE process so that the spread of every line is known (the protocol of
profiles/mask_overlap/bench_mask_overlap.py).

    python profiles/assign/bench_assign.py --out profiles/assign/bench_assign.json

Mask shapes: one image of 16 x 16 planes, 256 images with Poisson(7) planes on each side, 64 images of 100 x 100; each plane the
union of three rectangles or ellipses; ``R`` input sets in rotation.
  overlap         mask_overlap(a, b, ..., iou="iou", plan=plan) alone: the floor of both routes
  device          the same and assign_overlap(ov, plan=aplan): three kernels on one stream, tables prepared, nothing copied
  device.match    match_masks(a, b, ..., plan=plan): with the assignment's tables uploaded in the call and ``value`` (torch ops)
  assign          assign_overlap on a matrix that is already there: the assignment kernel alone (through its wrapper)
  host            mask_iou -> .cpu() -> SciPy per group -> the column of every row uploaded: what a caller did before
  host.scipy      the SciPy calls of that route alone, on matrices already on the host
Box shape: 5 000 scenes with Poisson(7) x Poisson(7) boxes, the boxes on the host as ``combine_coco_results`` holds them.
  box.device      match_boxes(all scenes) and one copy back (``Assignment.host()``): pass 3 with matching="device"
  box.host        per scene iou2d_matrix(...).cpu() and SciPy: pass 3 with matching="host"
Every line is warmed up and timed over ``steps`` calls between two HIP events with the host's clock beside them (``host_us``),
``steps`` raised until a run lasts ``--min-ms``, the lines alternated ``--reps`` times.  Before anything is timed the routes are
compared: every group's pairs exactly.  Prints one JSON document."""
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
p.add_argument("--min-ms", type=float, default=50.0, help="a timed run lasts at least this long")
p.add_argument("--shapes", default="1x16,256xP7,64x100,box5000xP7")
args = p.parse_args()
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402

import labelany3d_amd as la  # noqa: E402

H, W = 480, 640
NW = H * W // 32
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()


def make_bits(n, seed, chunk=256):
    """n planes made on the device - unions of three rectangles or ellipses - and packed, ``chunk`` planes at a time"""
    rs = np.random.RandomState(seed)
    vv = torch.arange(H, device=dev)[:, None]
    uu = torch.arange(W, device=dev)[None, :]
    parts, mb = [], None
    for j0 in range(0, max(n, 1), chunk):
        m = torch.zeros((min(chunk, n - j0), H, W), dtype=torch.bool, device=dev)
        for j in range(len(m)):
            for _ in range(3):
                cy, cx, hy, hx = rs.randint(0, H), rs.randint(0, W), rs.randint(8, H // 3), rs.randint(8, W // 3)
                if rs.rand() < 0.5:
                    m[j] |= ((vv - cy).abs() <= hy) & ((uu - cx).abs() <= hx)
                else:
                    m[j] |= ((vv - cy) / float(hy)) ** 2 + ((uu - cx) / float(hx)) ** 2 <= 1.0
        mb = la.pack_mask_bits(m.view(torch.uint8))
        parts.append(mb.bits)
    return la.MaskBits(torch.cat(parts), mb.H, mb.W, mb.frame_width)


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


def measure(lines):
    steps = {}
    for key, fn in lines.items():
        t, _ = time_device(fn, 2, 2)
        steps[key] = int(min(max(2, np.ceil(args.min_ms * 1e3 / max(t, 1.0))), 2000))
    raw = {key: [] for key in lines}
    for _ in range(args.reps):
        for key, fn in lines.items():
            raw[key].append(time_device(fn, steps[key], 2))
    return {key: dict(summarise(v), steps=steps[key]) for key, v in raw.items()}


def verdict(res, ours, theirs):
    """a win is claimed only where the medians differ by more than both spreads"""
    a, b = res[ours], res[theirs]
    gap = abs(a["median"] - b["median"])
    if gap <= max(a["spread"], b["spread"]):
        return "no difference beyond the spreads"
    return f"{ours} faster" if a["median"] < b["median"] else f"{theirs} faster"


def host_assign(flat, offsets, ca, cb, first_a):
    col = np.full(int(first_a[-1]), -1, np.int32)
    for g in range(len(ca)):
        if ca[g] and cb[g]:
            rows, cols = linear_sum_assignment(flat[offsets[g]:offsets[g + 1]].reshape(ca[g], cb[g]), maximize=True)
            col[first_a[g] + rows] = cols
    return col


def run_masks(name):
    imgs, per = name.split("x")
    P = int(imgs)
    if per.startswith("P"):
        ca, cb = np.random.RandomState(11).poisson(7, P).astype(np.int64), np.random.RandomState(12).poisson(7, P).astype(np.int64)
    else:
        ca = cb = np.full(P, int(per), np.int64)
    A, B = int(ca.sum()), int(cb.sum())
    R = 2 if (A + B) * NW * 4 > 64e6 else 4
    sa, sb = [make_bits(A, 1000 + 17 * r) for r in range(R)], [make_bits(B, 2000 + 17 * r) for r in range(R)]
    la_, lb_ = ca.tolist(), cb.tolist()
    first_a = np.concatenate([[0], np.cumsum(ca)])
    plan = la.mask_overlap_plan(sa[0], sb[0], la_, lb_)
    aplan = la.assign_plan(plan.offsets, la_, lb_)
    ovs = [la.mask_overlap(sa[r], sb[r], la_, lb_, iou="iou", plan=plan) for r in range(R)]
    host_m = [o.iou.cpu().numpy() for o in ovs]

    def host_route(k):
        ov = la.mask_overlap(sa[k % R], sb[k % R], la_, lb_, iou="iou", plan=plan)
        col = host_assign(ov.iou.cpu().numpy(), plan.offsets, ca, cb, first_a)
        return torch.as_tensor(col, device=dev)

    # the routes agree before anything is timed
    got = la.assign_overlap(ovs[0], plan=aplan)
    want = host_assign(host_m[0], plan.offsets, ca, cb, first_a)
    equal = bool((got.host()[0] == want).all() and (got.host()[2] == 0).all())
    zeros = float((host_m[0] == 0).mean()) if len(host_m[0]) else 0.0
    lines = {
        "overlap": lambda k: la.mask_overlap(sa[k % R], sb[k % R], la_, lb_, iou="iou", plan=plan),
        "device": lambda k: la.assign_overlap(la.mask_overlap(sa[k % R], sb[k % R], la_, lb_, iou="iou", plan=plan), plan=aplan),
        "device.match": lambda k: la.match_masks(sa[k % R], sb[k % R], la_, lb_, plan=plan),
        "assign": lambda k: la.assign_overlap(ovs[k % R], plan=aplan),
        "host": host_route,
        "host.scipy": lambda k: host_assign(host_m[k % R], plan.offsets, ca, cb, first_a),
    }
    res = measure(lines)
    del sa, sb, ovs
    torch.cuda.empty_cache()
    return dict(images=P, planes_a=A, planes_b=B, sets=R, pairs=int(plan.offsets[-1]), share_of_zero_iou=zeros, device_equals_scipy=equal,
                lines_us=res, verdict=verdict(res, "device", "host"))


def run_boxes(name):
    P = int(name[3:].split("x")[0])
    rs = np.random.RandomState(21)
    c0, c1 = rs.poisson(7, P).astype(np.int64), rs.poisson(7, P).astype(np.int64)

    def boxes(n):
        xy = rs.uniform(0, 500, (n, 2))
        return np.concatenate([xy, xy + rs.uniform(10, 200, (n, 2))], 1)

    b0, b1 = boxes(int(c0.sum())), boxes(int(c1.sum()))
    f0, f1 = np.concatenate([[0], np.cumsum(c0)]), np.concatenate([[0], np.cumsum(c1)])
    l0, l1 = c0.tolist(), c1.tolist()

    def device_route(k):
        m = la.match_boxes(b0, b1, l0, l1)
        return m.host()

    def host_route(k):
        col = np.full(len(b0), -1, np.int32)
        for g in range(P):
            if c0[g] and c1[g]:                                             # pass 3 of combine: one matrix, one copy, one SciPy call per scene
                iou = la.iou2d_matrix(b0[f0[g]:f0[g + 1]], b1[f1[g]:f1[g + 1]]).cpu().numpy()
                rows, cols = linear_sum_assignment(-iou)
                col[f0[g] + rows] = cols
        return col

    equal = bool((device_route(0)[0] == host_route(0)).all())
    res = measure({"box.device": device_route, "box.host": host_route})
    return dict(scenes=P, boxes0=int(c0.sum()), boxes1=int(c1.sum()), device_equals_scipy=equal, lines_us=res,
                verdict=verdict(res, "box.device", "box.host"))


doc = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, frame=[H, W], reps=args.reps, min_ms=args.min_ms,
           build=la._lib.lib.la3d_build_info().decode()[:32], shapes={})
for shape in args.shapes.split(","):
    doc["shapes"][shape] = run_boxes(shape) if shape.startswith("box") else run_masks(shape)
    print(shape, json.dumps({k: round(v["median"], 1) for k, v in doc["shapes"][shape]["lines_us"].items()}), doc["shapes"][shape]["verdict"],
          "equal" if doc["shapes"][shape]["device_equals_scipy"] else "NOT EQUAL", flush=True)
text = json.dumps(doc, indent=1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
print(json.dumps(doc))
