"""Measured lines of the ground plane from depth (include/la3d.h "ground plane: RANSAC plane fit"; RESULTS.md beside this file): resident
640 x 480 float32 frames - a floor under a pitched, rolled camera with a box on it and a band of 10000.0 fill, rendered by
tests/ground_plane_cases.scene -, grid step 4 (19200 grid pixels per frame), T = 256 trials, at P = 1 / 16 / 64 frames, alternated in ONE
process so that the spread of every line is known (the protocol of profiles/depth_gate/measure_depth_gate.py).

    python profiles/ground_plane/measure_ground_plane.py --out profiles/ground_plane

  select      plane_select_batch: grid pixels -> back-projected samples, pixel indices, counts
  ransac      plane_ransac_batch on those samples, subsets drawn on the device
  chain       ground_planes: select -> ransac, what a caller runs
  torch       the rule restated with torch on the same device and the same resident samples and subsets: the residuals of every trial as
              ONE (P,T,n) tensor operation, argmax over the counts, then a batched eigh over the masked covariance.  Its arithmetic may fuse
              and its ties may fall otherwise: a time comparator; how often it picks the kernels' trial is reported, not asserted
  numpy       the NumPy restatement of tests/ground_plane_cases.py on the host, on samples and subsets that are already there (no copy is
              timed), one run per batch size
Every device line is warmed up and timed over ``steps`` calls between two HIP events with the host's clock beside them (``host_us``),
``steps`` raised until a run lasts ``--min-ms``, the lines alternated ``--reps`` times.  Before anything is timed the chain is checked: every
frame fitted, its normal within 1e-4 rad of the rendered plane, and the kernels' decisions equal to the NumPy restatement's on frame 0.
Prints one JSON document and a markdown table."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
p = argparse.ArgumentParser()
p.add_argument("--out", default=None, help="directory for measure_ground_plane.json and table.md")
p.add_argument("--reps", type=int, default=3)
p.add_argument("--batches", default="1,16,64")
p.add_argument("--min-ms", type=float, default=60.0, help="a timed run lasts at least this long")
args = p.parse_args()
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import labelany3d_amd as la  # noqa: E402
from labelany3d_amd._lib import lib  # noqa: E402
from tests import ground_plane_cases as G  # noqa: E402

H, W, STEP, T, SEED = 480, 640, 4, 256, 7
THR, TILT, FAR = 0.01, 0.8, 100.0
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()


def frames(P):
    out = [G.scene(H, W, f=600.0, pitch=0.30 + 0.01 * (i % 8), roll=0.02 * ((i % 5) - 2), box_at=(0.1 * (i % 7) - 0.3, 3.0 + 0.1 * (i % 4)),
                   box_yaw=0.2 * (i % 6), sky_rows=40) for i in range(P)]
    return np.stack([s["depth"] for s in out]), out[0]["K"], np.stack([s["normal"] for s in out])


def torch_route(pts, counts, sub):
    """the rule on (P,n,3) samples with (P,T,3) subsets, residuals as one (P,T,n) tensor"""
    P, n, _ = pts.shape
    valid = torch.arange(n, device=dev)[None, :] < counts[:, None]
    idx = sub.long().clamp(0, n - 1)
    tri = torch.gather(pts[:, None].expand(P, T, n, 3), 2, idx[..., None].expand(P, T, 3, 3))
    a = tri[:, :, 0]
    w = torch.linalg.cross(tri[:, :, 1] - a, tri[:, :, 2] - a)
    s = (w * w).sum(-1)
    ok = (s > 0) & torch.isfinite(s) & (w[..., 1] ** 2 >= np.cos(TILT) ** 2 * s) & ((sub >= 0) & (sub < counts[:, None, None])).all(-1)
    e = torch.einsum("ptc,pnc->ptn", w, pts) - (w * a).sum(-1, keepdim=True)
    inl = (e * e <= (THR * THR) * s[..., None]) & valid[:, None, :]
    k = torch.where(ok, inl.sum(-1), torch.full((), -1, device=dev))
    best = k.argmax(1)
    m = torch.gather(inl, 1, best[:, None, None].expand(P, 1, n))[:, 0].to(pts.dtype)
    x = torch.nan_to_num(pts) * m[..., None]
    mu = x.sum(1) / m.sum(1, keepdim=True)
    c = (torch.nan_to_num(pts) - mu[:, None]) * m[..., None]
    vec = torch.linalg.eigh(c.transpose(1, 2) @ c).eigenvectors[..., 0]
    vec = torch.where(vec[:, 1:2] > 0, -vec, vec)
    return torch.cat([vec, -(vec * mu).sum(-1, keepdim=True)], 1), best, k.max(1).values


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


result = dict(build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0), frame=[H, W], step=STEP, trials=T, reps=args.reps,
              unit="us per call", lines={})
for P in (int(x) for x in args.batches.split(",")):
    depth_h, K, normals = frames(P)
    depth = torch.as_tensor(depth_h, device=dev)
    kw = dict(threshold=THR, max_trials=T, max_tilt=TILT)
    pts, pix, counts = la.plane_select_batch(depth, K, step=STEP, far=FAR)
    sub = la.ransac_subsets(counts, 3, T, SEED)
    gp = la.ground_planes(depth, K, step=STEP, far=FAR, seed=SEED, **kw)
    plane, status = gp.plane.cpu().numpy(), gp.status.cpu().numpy()
    assert (status == 0).all(), status                      # the chain, before anything is timed
    worst = max(G.angle(plane[i, :3], normals[i]) for i in range(P))
    assert worst <= 1e-4, worst
    pts_h, counts_h, sub_h = pts.cpu().numpy(), counts.cpu().numpy(), sub.cpu().numpy()
    ref0 = G.ransac_ref(pts_h[0], int(counts_h[0]), sub_h[0], THR, 0.0, G.cos2(TILT))
    assert int(gp.best_trial[0]) == ref0["best_trial"] and int(gp.k_trial[0]) == ref0["k_trial"] and G.angle(plane[0, :3], ref0["plane"][:3]) <= 1e-9
    t_plane, t_best, t_k = torch_route(pts, counts, sub)
    agree = dict(best_trial=float((t_best.cpu().numpy() == gp.best_trial.cpu().numpy()).mean()),
                 worst_angle_to_kernel=float(max(G.angle(a, b) for a, b in zip(t_plane.cpu().numpy()[:, :3], plane[:, :3]))))
    lines = {
        "select": lambda k: la.plane_select_batch(depth, K, step=STEP, far=FAR),
        "ransac": lambda k: la.plane_ransac_batch(pts, counts, seed=SEED, **kw),
        "chain": lambda k: la.ground_planes(depth, K, step=STEP, far=FAR, seed=SEED, **kw),
        "torch": lambda k: torch_route(pts, counts, sub),
    }
    nsteps = {}
    for name, fn in lines.items():                          # a run lasts at least --min-ms: from a pilot
        ev, host = time_device(fn, 2, 1)
        nsteps[name] = max(2, int(np.ceil(args.min_ms * 1e3 / max(ev, host, 1e-3))))
    times = {k: [] for k in lines}
    for _ in range(args.reps):
        for name, fn in lines.items():
            times[name].append(time_device(fn, nsteps[name], max(nsteps[name] // 10, 1)))
    res = {k: summarise(v) for k, v in times.items()}
    t0 = time.perf_counter()
    for i in range(P):
        G.ransac_ref(pts_h[i], int(counts_h[i]), sub_h[i], THR, 0.0, G.cos2(TILT))
    res["numpy"] = dict(median=(time.perf_counter() - t0) * 1e6, runs=1)
    for k in ("torch", "numpy"):
        res[k]["over_ransac"] = res[k]["median"] / res["ransac"]["median"]
    res["inputs"] = dict(samples_per_frame=float(counts_h.mean()), cap=int(pts.shape[1]), worst_angle_to_truth=worst)
    res["torch_agreement"] = agree
    res["steps"] = nsteps
    result["lines"][str(P)] = res
    print(P, {k: round(v["median"], 1) for k, v in res.items() if isinstance(v, dict) and "median" in v}, agree, file=sys.stderr, flush=True)
    del depth, pts, pix, counts, sub, gp
    torch.cuda.empty_cache()

rows = ["| P | select | ransac | chain (`ground_planes`) | torch restatement | NumPy restatement (host) |", "|---|---|---|---|---|---|"]
for P, r in result["lines"].items():
    cell = lambda k: f"{r[k]['median']:.1f} ({r[k]['min']:.1f} .. {r[k]['max']:.1f})"   # noqa: E731
    rows.append(f"| {P} | {cell('select')} | {cell('ransac')} | {cell('chain')} | {cell('torch')} = {r['torch']['over_ransac']:.1f} x ransac | "
                f"{r['numpy']['median']:.0f} = {r['numpy']['over_ransac']:.0f} x ransac |")
table = "\n".join(rows)
doc = json.dumps(result, indent=1)
if args.out:
    with open(os.path.join(args.out, "measure_ground_plane.json"), "w") as f:
        f.write(doc + "\n")
    with open(os.path.join(args.out, "table.md"), "w") as f:
        f.write(table + "\n")
print(doc)
print(table)
