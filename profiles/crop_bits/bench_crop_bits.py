"""Measured lines of the crop-space packer (include/la3d.h "crop-space masks as bit planes"; RESULTS.md beside this file): S = 256
crops -> the ``MaskBits`` of 640 x 480 frames, against the two routes a caller had before, alternated in ONE process so that the
spread of every line is known (the protocol of profiles/annotation_bits/bench_annotation_bits.py).

    python profiles/crop_bits/bench_crop_bits.py --out profiles/crop_bits/bench_crop_bits.json

Inputs: B = 1 / 16 / 256 / 1024 objects of 8..300 x 8..330 px in a 640 x 480 frame, cropped the way ``crop_object`` (reference
src/util.py:140-160) crops them - side_len = int(max(w, h) / 0.7), offsets x + (w - side_len) / 2 (half of them end in .5), scale
256 / side_len - with an ellipse as the mask of the 256 x 256 crop; three batches in rotation.
  new.resident  pack_crop_bits on resident crops and resident placement rows (what a completion network on the device leaves)
  new.host      pack_crop_bits on host crops and host parameters: crop_placement, the upload of 65 536 B per crop, the kernel
  a.restore     route (a), host: the NumPy restatement of restore_mask_from_crop per instance -> (B, 480, 640) u8
  a.upload      route (a): that array to the device (pageable memory, as a caller holds it)
  a.pack        route (a) / (b): pack_mask_bits on the resident (B, 480, 640) planes
  b.restore     route (b), device: the same rule by torch indexing on resident crops -> (B, 480, 640) u8
  b.total       route (b): b.restore then pack_mask_bits
``model_MB`` of new.resident = B * (S * S * pixel_step + H * W_out / 8) bytes, ``model_GBps`` = that over the median time.
Every line is warmed up and timed over ``steps`` calls - device lines between two HIP events, with the host's clock beside them
(``host_us``: where it equals the event time the line is bound by the Python wrapper), host lines (a.restore, a.upload, new.host) on
the host's clock around a loop that ends in a synchronise -, ``steps`` raised until a run lasts ``--min-ms``, the lines alternated
``--reps`` times.  Before anything is timed the three routes are compared bit for bit.  Prints one JSON document."""
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
args = p.parse_args()
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import labelany3d_amd as la  # noqa: E402
from labelany3d_amd._lib import lib  # noqa: E402

H, W, S, R = 480, 640, 256, 3
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()


def make_batch(B, seed):
    rs = np.random.RandomState(seed)
    w, h = rs.randint(8, 301, B), rs.randint(8, 331, B)
    x, y = (rs.rand(B) * (W - w)).astype(np.int64), (rs.rand(B) * (H - h)).astype(np.int64)
    side = (np.maximum(w, h) / 0.7).astype(np.int64)
    params = np.stack([x + (w - side) / 2, y + (h - side) / 2, S / side], 1)
    yy, xx = np.mgrid[0:S, 0:S]
    rx, ry = (w / side * S / 2)[:, None, None], (h / side * S / 2)[:, None, None]
    crops = ((((xx[None] - S / 2 + 0.5) / rx) ** 2 + ((yy[None] - S / 2 + 0.5) / ry) ** 2) <= 1.0).astype(np.uint8)
    return crops, params


def restore_host(crops, params):
    """route (a): the rule of restore_mask_from_crop in NumPy, one instance at a time, as the reference's loop does"""
    out = np.zeros((len(crops), H, W), np.uint8)
    for n, (c, (ox, oy, s)) in enumerate(zip(crops, params.tolist())):
        side, x1, y1 = int(S / s), int(round(ox)), int(round(oy))
        if side <= 0:
            continue
        ifx = 1.0 / (side / S)
        u0, u1, v0, v1 = max(x1, 0), min(x1 + side, W), max(y1, 0), min(y1 + side, H)
        if u0 >= u1 or v0 >= v1:
            continue
        sx = np.minimum(np.floor(np.arange(u0 - x1, u1 - x1) * ifx).astype(np.int64), S - 1)
        sy = np.minimum(np.floor(np.arange(v0 - y1, v1 - y1) * ifx).astype(np.int64), S - 1)
        out[n, v0:v1, u0:u1] = c[np.ix_(sy, sx)]
    return out


def restore_torch(crops_d, place_d):
    """route (b): the same rule by torch indexing on the device, the whole batch at once -> (B, H, W) u8"""
    B = crops_d.shape[0]
    x1, y1, side = place_d[:, 0:1].long(), place_d[:, 1:2].long(), place_d[:, 2:3].long()
    ifx = 1.0 / (side.double() / S)
    du, dv = torch.arange(W, device=dev)[None] - x1, torch.arange(H, device=dev)[None] - y1
    inu, inv = (du >= 0) & (du < side), (dv >= 0) & (dv < side)
    sx = torch.clamp(torch.floor(du.clamp(min=0).double() * ifx).long(), max=S - 1)
    sy = torch.clamp(torch.floor(dv.clamp(min=0).double() * ifx).long(), max=S - 1)
    got = crops_d[torch.arange(B, device=dev)[:, None, None], sy[:, :, None], sx[:, None, :]]
    return got * (inv[:, :, None] & inu[:, None, :]).to(torch.uint8)


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


result = dict(build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0), frame=[H, W], S=S, reps=args.reps, lines={})
for B in [int(x) for x in args.batches.split(",")]:
    bs = []
    for r in range(R):
        crops, params = make_batch(B, 4321 + r)
        bs.append(dict(crops=crops, params=params, crops_d=torch.as_tensor(crops, device=dev),
                       place_d=torch.as_tensor(la.crop_placement(params, S), device=dev),
                       planes=torch.empty((B, H * W // 32), dtype=torch.int32, device=dev), area=torch.empty(B, dtype=torch.int32, device=dev)))
    b0 = bs[0]
    host_u8 = [restore_host(b["crops"], b["params"]) for b in bs]
    dev_u8 = [torch.as_tensor(m, device=dev) for m in host_u8]
    # the three routes give the same planes, bit for bit
    new = la.pack_crop_bits(b0["crops_d"], b0["place_d"], (W, H)).bits
    assert torch.equal(restore_torch(b0["crops_d"], b0["place_d"]), dev_u8[0])
    assert torch.equal(new, la.pack_mask_bits(dev_u8[0]).bits) and torch.equal(new, la.pack_crop_bits(b0["crops"], b0["params"], (W, H)).bits)
    assert int(dev_u8[0].sum()) > 0
    device_lines = {
        "new.resident": lambda k: la.pack_crop_bits(bs[k % R]["crops_d"], bs[k % R]["place_d"], (W, H), out=bs[k % R]["planes"], area=bs[k % R]["area"]),
        "a.pack": lambda k: la.pack_mask_bits(dev_u8[k % R], out=bs[k % R]["planes"]),
        "b.restore": lambda k: restore_torch(bs[k % R]["crops_d"], bs[k % R]["place_d"]),
        "b.total": lambda k: la.pack_mask_bits(restore_torch(bs[k % R]["crops_d"], bs[k % R]["place_d"]), out=bs[k % R]["planes"]),
    }
    host_lines = {
        "new.host": lambda k: la.pack_crop_bits(bs[k % R]["crops"], bs[k % R]["params"], (W, H), out=bs[k % R]["planes"], area=bs[k % R]["area"]),
        "a.restore": lambda k: restore_host(bs[k % R]["crops"], bs[k % R]["params"]),
        "a.upload": lambda k: torch.as_tensor(host_u8[k % R], device=dev),
    }
    lines = {**{k: (f, time_device) for k, f in device_lines.items()}, **{k: (f, time_host) for k, f in host_lines.items()}}
    nsteps = {}
    for name, (fn, timer) in lines.items():   # a run lasts at least --min-ms: from a pilot of two calls
        ev, host = timer(fn, 2, 1)
        nsteps[name] = max(2, int(np.ceil(args.min_ms * 1e3 / max(ev, host, 1e-3))))
    times = {k: [] for k in lines}
    for _ in range(args.reps):
        for name, (fn, timer) in lines.items():
            times[name].append(timer(fn, nsteps[name], max(nsteps[name] // 10, 1)))
    res = {k: summarise(v) for k, v in times.items()}
    mbytes = B * (S * S * 1 + H * W // 8)
    res["new.resident"].update(model_MB=mbytes / 1e6, model_GBps=mbytes / (res["new.resident"]["median"] * 1e-6) / 1e9,
                               b_total_over_new=res["b.total"]["median"] / res["new.resident"]["median"],
                               beats_route_b=bool(res["new.resident"]["max"] <= res["b.total"]["min"]))
    res["a.total"] = dict(median=res["a.restore"]["median"] + res["a.upload"]["median"] + res["a.pack"]["median"], note="sum of the medians of its three parts")
    res["new.host"].update(a_total_over_new=res["a.total"]["median"] / res["new.host"]["median"])
    res["steps"] = nsteps
    result["lines"][f"B={B}"] = res
    print(f"B={B}", {k: round(v["median"], 1) for k, v in res.items() if isinstance(v, dict) and "median" in v}, flush=True)
    del bs, b0, host_u8, dev_u8, new, lines, device_lines, host_lines
    torch.cuda.empty_cache()

text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
