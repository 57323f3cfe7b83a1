"""Measured lines of the instance point clouds (include/la3d.h "instance point clouds"; RESULTS.md beside this file): the new call
against the route a caller had before it existed, alternated in ONE process so that the spread of every line is known.

    python profiles/instance_points/bench_instance_points.py --out profiles/instance_points/bench_instance_points.json

Inputs: B = 1 / 16 / 256 / 1024 instances of 640 x 480 with config-2 masks (bench.make_inputs' rectangles of 8..300 x 8..330 px),
three resident batches in rotation, private depth planes (one per instance) and one shared plane (image_index = 0).
  new.u8 / new.bits   instance_points(depth, masks | MaskBits, K, capacity=<rows>) - both stages, never synchronises
  old                 unproject(planes, K), then points[plane][mask] per instance in torch (one gather launch and one host
                      synchronisation per instance)
The batch ``frames`` is the frames form: 256 images of the project's mixed-size mix, 7 instances each (1792 rows), resident
``PackedFrames`` and ``FrameBits``, one camera per image
  frames.bits         instance_points_frames(pf, fb, K, capacity=<rows>) - both stages; no other route is timed for it
Every line is warmed up, timed between two HIP events over ``steps`` calls, and the lines are alternated ``--reps`` times.
``model_MB``: the bytes the new call has to move at least - mask bytes + the 128-byte depth lines that hold a mask pixel + 24 B per
point -, from the rectangles; ``model_GBps`` = that over the median time; ``writer_GBps``: a device fill of 1 GiB timed in the same
process; ``share_of_writer`` = model_GBps / writer_GBps.  Prints one JSON document."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
p = argparse.ArgumentParser()
p.add_argument("--out", default=None)
p.add_argument("--reps", type=int, default=3)
p.add_argument("--batches", default="1,16,256,1024,frames")
p.add_argument("--quick", action="store_true", help="a fifth of the steps (rehearsal)")
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
NEW_STEPS = {1: 500, 16: 300, 256: 50, 1024: 20}
OLD_STEPS = {1: 100, 16: 30, 256: 4, 1024: 2}


def model_bytes(rects, mask_bytes_per_instance):
    """mask bytes + touched 128-byte depth lines + 24 B per point (rows are 640 floats: lines never straddle rows)"""
    r0, c0, hh, ww = rects
    lines = -(-(c0 + ww) // 32) - c0 // 32
    return int(len(hh) * mask_bytes_per_instance + (hh * lines).sum() * 128 + (hh * ww).sum() * 24)


def make_batches(B):
    out = []
    for r in range(R):
        depth, masks, K, npix, rects = bench.make_inputs(B, dev, 1234 + r)
        out.append(dict(depth=depth, masks=masks, mbool=masks.view(torch.bool), bits=la.pack_mask_bits(masks), K=K, rows=int(npix), rects=rects,
                        zero=torch.zeros(B, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    return out


def new_route(b, src, shared):
    d = b["depth"][:1] if shared else b["depth"]
    return la.instance_points(d, b[src], b["K"], image_index=b["zero"] if shared else None, capacity=b["rows"])


def old_route(b, shared):
    pts = la.unproject(b["depth"][:1] if shared else b["depth"], b["K"])
    m = b["mbool"]
    return [pts[0 if shared else n][m[n]] for n in range(m.shape[0])]


def time_line(fn, steps, warmup):
    for k in range(warmup):
        fn(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(st)
    for k in range(steps):
        fn(warmup + k)
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps   # us per call


def summarise(v):
    v = sorted(v)
    return dict(median=float(np.median(v)), min=v[0], max=v[-1], spread=v[-1] - v[0], runs=v)


COCO_SIZES = [(480, 640), (640, 480), (427, 640), (640, 427), (426, 640), (428, 640), (375, 500), (500, 375), (333, 500), (425, 640),
              (480, 480), (640, 640), (360, 640), (500, 333), (612, 612), (424, 640), (334, 500), (512, 640)]


def coco_mix(images, seed):
    """the sizes of ``images`` images: share 1 / rank over COCO_SIZES, in a seeded arrival order (the project's mixed-size mix,
    profiles/open_bits_frames/bench_open_bits_frames.py, restated here because that script runs on import)"""
    rs = np.random.RandomState(seed)
    share = 1.0 / np.arange(1, len(COCO_SIZES) + 1)
    share /= share.sum()
    n = np.maximum(1, np.round(share * images).astype(int))
    n[0] += images - n.sum()
    sizes = [s for s, k in zip(COCO_SIZES, n) for _ in range(k)]
    return [sizes[i] for i in rs.permutation(len(sizes))]


def make_stacks(sizes, per, seed):
    """one (per, h, w) uint8 stack per image, made on the device: unions of three rectangles or ellipses"""
    rs = np.random.RandomState(seed)
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
        out.append(m.view(torch.uint8))
    return out


def frames_lines(images=256, per=7, steps=40):
    """the frames form on the mixed-size mix; before anything is timed the rows of three instances are compared with the uniform call"""
    sizes = coco_mix(images, 7)
    rs = np.random.RandomState(5)
    depth = [rs.uniform(0.5, 10.0, hw).astype(np.float32) for hw in sizes]
    pf = la.pack_frames(depth, device=dev)
    K = np.stack([np.array([[0.8 * w, 0.0, w / 2.0], [0.0, 0.9 * w, h / 2.0], [0.0, 0.0, 1.0]]) for h, w in sizes])
    sets = []
    for r in range(2):
        stacks = make_stacks(sizes, per, 4100 + r)
        fb = la.pack_mask_bits_frames(la.pack_mask_frames(stacks))
        sets.append(dict(stacks=stacks, fb=fb, rows=int(fb.area.sum())))
    ip = la.instance_points_frames(pf, sets[0]["fb"], K, capacity=sets[0]["rows"])
    torch.cuda.synchronize()
    assert int(ip.offsets[-1]) == sets[0]["rows"] and int((ip.status != 0).sum()) == 0
    off = ip.offsets.cpu().numpy()
    for g in (0, images // 2, images - 1):
        one = la.instance_points(torch.as_tensor(depth[g], device=dev), sets[0]["stacks"][g], K[g])
        assert torch.equal(torch.nan_to_num(ip.points[off[g * per]:off[(g + 1) * per]], nan=-7.0), torch.nan_to_num(one.points, nan=-7.0)), g
    fn = lambda k: la.instance_points_frames(pf, sets[k % 2]["fb"], K, capacity=sets[k % 2]["rows"])  # noqa: E731
    st_ = max(steps // (5 if args.quick else 1), 2)
    res = {"frames.bits": summarise([time_line(fn, st_, max(st_ // 10, 1)) for _ in range(args.reps)])}
    res["steps"] = dict(new=st_)
    res["rows"] = float(np.mean([d["rows"] for d in sets]))
    res["images"], res["distinct_sizes"] = images, len(set(sizes))
    return res


def writer_rate():
    buf = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    t = time_line(lambda k: buf.zero_(), 20, 3)
    return buf.numel() * 4 / (t * 1e-6) / 1e9


result = dict(build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0), frame=[H, W], reps=args.reps,
              writer_GBps=writer_rate(), lines={})
for B in args.batches.split(","):
    if B == "frames":
        result["lines"]["frames"] = frames_lines()
        print("frames", {"frames.bits": round(result["lines"]["frames"]["frames.bits"]["median"], 1)}, flush=True)
        torch.cuda.empty_cache()
        continue
    B = int(B)
    batches = make_batches(B)
    scale = 5 if args.quick else 1
    ns, os_ = max(NEW_STEPS.get(B, 20) // scale, 2), max(OLD_STEPS.get(B, 2) // scale, 1)
    for shared in (False, True):
        tag = f"B={B}.{'shared' if shared else 'private'}"
        # the two routes give the same rows, bit for bit
        b0 = batches[0]
        want = torch.cat(old_route(b0, shared))
        for src in ("masks", "bits"):
            got = new_route(b0, src, shared)
            torch.cuda.synchronize()
            assert int(got.offsets[-1]) == b0["rows"] and int((got.status != 0).sum()) == 0
            assert torch.equal(torch.nan_to_num(got.points, nan=-7.0), torch.nan_to_num(want, nan=-7.0)), (tag, src)
        del want, got
        lines = {"new.u8": (lambda k, s=shared: new_route(batches[k % R], "masks", s), ns),
                 "new.bits": (lambda k, s=shared: new_route(batches[k % R], "bits", s), ns),
                 "old": (lambda k, s=shared: old_route(batches[k % R], s), os_)}
        times = {k: [] for k in lines}
        for _ in range(args.reps):
            for name, (fn, steps) in lines.items():
                times[name].append(time_line(fn, steps, max(steps // 10, 1)))
        res = {k: summarise(v) for k, v in times.items()}
        for src, per in (("new.u8", H * W), ("new.bits", H * W // 8)):
            mb = float(np.mean([model_bytes(b["rects"], per) for b in batches]))
            res[src].update(model_MB=mb / 1e6, model_GBps=mb / (res[src]["median"] * 1e-6) / 1e9)
            res[src]["share_of_writer"] = res[src]["model_GBps"] / result["writer_GBps"]
            res[src]["old_over_new"] = res["old"]["median"] / res[src]["median"]
            res[src]["not_slower_than_old"] = bool(res[src]["max"] <= res["old"]["min"])
        res["steps"] = dict(new=ns, old=os_)
        res["rows"] = float(np.mean([b["rows"] for b in batches]))
        result["lines"][tag] = res
        print(tag, {k: round(v["median"], 1) for k, v in res.items() if isinstance(v, dict) and "median" in v}, flush=True)
    del batches
    torch.cuda.empty_cache()

text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
