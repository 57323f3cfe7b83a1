"""Measured lines of the frames call (DESIGN.md section 5 "images of different sizes in one call"), every comparison alternated in ONE
process so that the run-to-run spread of each line is known.

    python profiles/frames/measure_frames.py --out profiles/frames/measure_frames.json          # this tree
    python profiles/frames/measure_frames.py --root <checkout of the parent commit> --out ...    # the parent's uniform lines only

(a) ``coco_mix``: 256 images over 18 COCO frame sizes with a Zipf-like share per size (the most frequent size holds about a quarter of
    the images, the tail sizes one or two), ~7 instances per image (Poisson), ellipses of log-uniform area as polygons (75 %) or
    run lengths (25 %), the fused filter on and the annotation areas as ``area_hint`` - what ``fit_scenes`` feeds.  Fitted as ONE
    frames call per annotation kind, and - same data, same process - as the parent's one call per size group and kind
    (``la3d_fit_instances_ex`` with ``frame_width``).  Both are pure enqueues of prepared argument blocks on resident inputs.
(b) ``uniform_1024``: BASELINE config 2's generator (bench.make_inputs: 1024 instances of 480x640, private depth planes) as run lengths
    and as 4-vertex polygons through the existing entry - the lines to hold against the parent's -, and the same batch through the
    frames entry with a table of 1024 equal frames, with and without ``area_hint`` (a frames call takes its size-balanced launch order
    from the hint only): what the table look-up costs.
Three resident input batches in rotation (seeds + 0 / 1 / 2), 5 warm-up + 20 timed steps per line between two HIP events, the lines
alternated ``--reps`` times (default 6); median, min, max and spread (max - min) of every line are reported."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

p = argparse.ArgumentParser()
p.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
p.add_argument("--out", default=None)
p.add_argument("--reps", type=int, default=6)
p.add_argument("--steps", type=int, default=20)
p.add_argument("--warmup", type=int, default=5)
p.add_argument("--images", type=int, default=256)
args = p.parse_args()
sys.path.insert(0, args.root)

import torch  # noqa: E402

import bench  # noqa: E402
from labelany3d_amd import batched, masks  # noqa: E402
from labelany3d_amd._lib import check, lib  # noqa: E402

R = 3
HAVE_FRAMES = hasattr(lib, "la3d_fit_instances_frames")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
up = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), device=dev) if dt is None else torch.as_tensor(np.ascontiguousarray(a), device=dev).to(dt)  # noqa: E731
FLT = {"boundary_threshold": 10, "scale_threshold": 100}

# (H, W) of COCO images by falling frequency: 640x480 and 480x640 hold most, a long tail follows
COCO_SIZES = [(480, 640), (640, 480), (427, 640), (640, 427), (426, 640), (428, 640), (375, 500), (500, 375), (333, 500), (425, 640),
              (480, 480), (640, 640), (360, 640), (500, 333), (612, 612), (424, 640), (334, 500), (512, 640)]


def padded(w):
    return (w + 31) // 32 * 32


def rle_of(m):
    flat = m.ravel(order="F")
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return ([0] + counts) if flat[0] else counts


def coco_mix(seed):
    """images, their sizes, and the annotations of both kinds with image index and area"""
    rs = np.random.RandomState(seed)
    share = 1.0 / np.arange(1, len(COCO_SIZES) + 1)
    share /= share.sum()
    n = np.maximum(1, np.round(share * args.images).astype(int))
    n[0] += args.images - n.sum()
    sizes = [s for s, k in zip(COCO_SIZES, n) for _ in range(k)]
    order = rs.permutation(len(sizes))
    sizes = [sizes[i] for i in order]                                   # arrival order: sizes mixed
    depth, K = [], []
    rle = dict(counts=[], offsets=[0], img=[], area=[])
    poly = dict(xy=[], ring=[0], inst=[0], img=[], area=[])
    for pi, (h, w) in enumerate(sizes):
        vv, uu = np.mgrid[0:h, 0:w]
        depth.append((rs.uniform(2, 6) + rs.uniform(-1e-3, 1e-3) * uu + rs.uniform(0, 3e-3) * vv + 0.02 * rs.randn(h, w)).astype(np.float32))
        f = rs.uniform(450, 650)
        K.append([[f, 0.0, w / 2], [0.0, f, h / 2], [0.0, 0.0, 1.0]])
        for _ in range(max(1, rs.poisson(7.0))):
            area = np.exp(rs.uniform(np.log(200), np.log(90000)))
            asp = np.exp(rs.uniform(-0.6, 0.6))
            hh, ww = min(np.sqrt(area * asp), 0.9 * h), min(np.sqrt(area / asp), 0.9 * w)
            cy, cx = rs.uniform(hh / 2 + 11, max(h - hh / 2 - 11, hh / 2 + 12)), rs.uniform(ww / 2 + 11, max(w - ww / 2 - 11, ww / 2 + 12))
            if rs.rand() < 0.25:
                m = (((vv - cy) / (hh / 2)) ** 2 + ((uu - cx) / (ww / 2)) ** 2) <= 1.0
                rle["counts"] += rle_of(m); rle["offsets"].append(len(rle["counts"])); rle["img"].append(pi); rle["area"].append(int(m.sum()))
            else:
                ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
                poly["xy"].append(np.stack([cx + ww / 2 * np.cos(ang), cy + hh / 2 * np.sin(ang)], 1).astype(np.int32))
                poly["ring"].append(poly["ring"][-1] + 24); poly["inst"].append(len(poly["ring"]) - 1)
                poly["img"].append(pi); poly["area"].append(int(np.pi * hh * ww / 4))
    return dict(sizes=sizes, depth=depth, K=np.asarray(K), rle=rle, poly=poly)


def block(f, B, H, W, depth, planes, K, nk, **kw):
    return batched._fit_args(B, H, W, ptr(depth), planes, ptr(K), nk, ptr(f.boxes[0]), ptr(f.status[0]), ptr(f.aux[0]), ptr(f.workspace[0]),
                             C.c_void_p(st.cuda_stream), **kw)


def prepare_mixed(mix):
    """one frames call per annotation kind"""
    pf = masks.pack_frames(mix["depth"], device=dev)
    K = up(mix["K"])
    calls, keep = [], [pf, K]
    for kind in ("rle", "poly"):
        g = mix[kind]
        B = len(g["img"])
        f = batched.InstanceFitter(B, pf.H, pf.W, dev)
        ii, ah, stats = up(np.asarray(g["img"], np.int32)), up(np.asarray(g["area"], np.int32)), torch.zeros((B, 4), dtype=torch.int32, device=dev)
        if kind == "rle":
            c, o = up(np.asarray(g["counts"], np.int32)), up(np.asarray(g["offsets"], np.int64))
            a = block(f, B, pf.H, pf.W, pf.depth, 1, K, len(K), rle=(ptr(c), ptr(o)), image_index=ptr(ii), area_hint=ptr(ah), filter=FLT, stats=ptr(stats))
            keep += [c, o]
        else:
            xy, ro, ir = up(np.concatenate(g["xy"])), up(np.asarray(g["ring"], np.int64)), up(np.asarray(g["inst"], np.int64))
            a = block(f, B, pf.H, pf.W, pf.depth, 1, K, len(K), poly=(ptr(xy), ptr(ro), ptr(ir)), image_index=ptr(ii), area_hint=ptr(ah), filter=FLT,
                      stats=ptr(stats))
            keep += [xy, ro, ir]
        keep += [f, ii, ah, stats]
        calls.append((a, f, B))
    table, P = pf.table, len(mix["sizes"])

    def run():
        for a, _, _ in calls:
            check(lib.la3d_fit_instances_frames(C.byref(a), ptr(table), P), "frames")
    return run, calls, keep


def prepare_grouped(mix):
    """the parent's way: one call per frame size and annotation kind, depth rows padded to the next multiple of 32"""
    calls, keep = [], []
    for size in sorted(set(mix["sizes"])):
        imgs = [i for i, s in enumerate(mix["sizes"]) if s == size]
        local = {i: n for n, i in enumerate(imgs)}
        h, w = size
        d = np.zeros((len(imgs), h, padded(w)), np.float32)
        for n, i in enumerate(imgs):
            d[n, :, :w] = mix["depth"][i]
        d, K = up(d), up(mix["K"][imgs])
        keep += [d, K]
        for kind in ("rle", "poly"):
            g = mix[kind]
            sel = [n for n, i in enumerate(g["img"]) if i in local]
            if not sel:
                continue
            B = len(sel)
            f = batched.InstanceFitter(B, h, padded(w), dev)
            ii = up(np.asarray([local[g["img"][n]] for n in sel], np.int32))
            ah, stats = up(np.asarray([g["area"][n] for n in sel], np.int32)), torch.zeros((B, 4), dtype=torch.int32, device=dev)
            kw = dict(image_index=ptr(ii), area_hint=ptr(ah), filter=FLT, stats=ptr(stats), frame_width=0 if padded(w) == w else w)
            if kind == "rle":
                parts = [g["counts"][g["offsets"][n]:g["offsets"][n + 1]] for n in sel]
                c, o = up(np.concatenate(parts).astype(np.int32)), up(np.concatenate([[0], np.cumsum([len(q) for q in parts])]).astype(np.int64))
                a = block(f, B, h, padded(w), d, len(imgs), K, len(imgs), rle=(ptr(c), ptr(o)), **kw)
                keep += [c, o]
            else:
                xy = up(np.concatenate([g["xy"][n] for n in sel]))
                ro, ir = up(np.arange(B + 1, dtype=np.int64) * 24), up(np.arange(B + 1, dtype=np.int64))
                a = block(f, B, h, padded(w), d, len(imgs), K, len(imgs), poly=(ptr(xy), ptr(ro), ptr(ir)), **kw)
                keep += [xy, ro, ir]
            if len(imgs) == 1:
                a.depth_plane_stride = 0
            keep += [f, ii, ah, stats]
            calls.append((a, f, B, kind, sel))

    def run():
        for a, *_ in calls:
            check(lib.la3d_fit_instances_ex(C.byref(a)), "grouped")
    return run, calls, keep


def time_line(fn):
    for k in range(args.warmup):
        fn(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(st)
    for k in range(args.steps):
        fn(args.warmup + k)
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.steps   # us per step


def summarise(v):
    v = sorted(v)
    return dict(median=float(np.median(v)), min=v[0], max=v[-1], spread=v[-1] - v[0], runs=v)


def alternate(lines):
    times = {k: [] for k in lines}
    for _ in range(args.reps):
        for name, fn in lines.items():
            times[name].append(time_line(fn))
    return {k: summarise(v) for k, v in times.items()}


result = dict(tree=os.path.relpath(args.root), have_frames=HAVE_FRAMES, build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0),
              steps=args.steps, warmup=args.warmup, reps=args.reps)

# ---- (b) uniform lines at B = 1024 of 480 x 640 ------------------------------------------------------------------------------------
H, W, B = bench.H, bench.W, 1024
ub = []
for r in range(R):
    depth, mk, K, npix, rects = bench.make_inputs(B, dev, 1234 + r)
    r0, c0, hh, ww = (np.asarray(v).astype(np.int64) for v in rects)
    counts, offsets = [], [0]
    for i in range(B):
        c = [int(c0[i]) * H + int(r0[i])]
        for j in range(int(ww[i])):
            c += [int(hh[i]), H - int(hh[i])]
        c[-1] = H * W - sum(c[:-1])
        counts += c
        offsets.append(len(counts))
    xy = np.stack([np.stack([c0, r0], 1), np.stack([c0 + ww - 1, r0], 1), np.stack([c0 + ww - 1, r0 + hh - 1], 1), np.stack([c0, r0 + hh - 1], 1)], 1)
    del mk
    ub.append(dict(depth=depth, K=K, ah=up((hh * ww).astype(np.int32)), c=up(np.asarray(counts, np.int32)), o=up(np.asarray(offsets, np.int64)), xy=up(xy.reshape(-1, 2).astype(np.int32)),
                   ro=up(np.arange(B + 1, dtype=np.int64) * 4), ir=up(np.arange(B + 1, dtype=np.int64)), ii=up(np.arange(B, dtype=np.int32))))
fu = batched.InstanceFitter(B, H, W, dev)
rle_blocks = [block(fu, B, H, W, b["depth"], B, b["K"], 1, rle=(ptr(b["c"]), ptr(b["o"]))) for b in ub]
poly_blocks = [block(fu, B, H, W, b["depth"], B, b["K"], 1, poly=(ptr(b["xy"]), ptr(b["ro"]), ptr(b["ir"]))) for b in ub]
lines = {"rle_uniform": lambda k: check(lib.la3d_fit_instances_ex(C.byref(rle_blocks[k % R])), "rle"),
         "poly_uniform": lambda k: check(lib.la3d_fit_instances_ex(C.byref(poly_blocks[k % R])), "poly")}
if HAVE_FRAMES:
    tab = np.zeros(B, masks.FRAME_DTYPE)
    tab["depth_offset"], tab["H"], tab["W"], tab["frame_width"] = np.arange(B, dtype=np.int64) * H * W, H, W, W
    tab_d = up(tab.view(np.int32).reshape(B, 6))
    fr_rle = [block(fu, B, H, W, b["depth"], 1, b["K"], 1, rle=(ptr(b["c"]), ptr(b["o"])), image_index=ptr(b["ii"])) for b in ub]
    fr_poly = [block(fu, B, H, W, b["depth"], 1, b["K"], 1, poly=(ptr(b["xy"]), ptr(b["ro"]), ptr(b["ir"])), image_index=ptr(b["ii"])) for b in ub]
    # (without a hint a frames call runs in the plain launch order; the uniform lines order themselves by their own estimate)
    fr_rle_h = [block(fu, B, H, W, b["depth"], 1, b["K"], 1, rle=(ptr(b["c"]), ptr(b["o"])), image_index=ptr(b["ii"]), area_hint=ptr(b["ah"])) for b in ub]
    fr_poly_h = [block(fu, B, H, W, b["depth"], 1, b["K"], 1, poly=(ptr(b["xy"]), ptr(b["ro"]), ptr(b["ir"])), image_index=ptr(b["ii"]), area_hint=ptr(b["ah"]))
                 for b in ub]
    rle_h = [block(fu, B, H, W, b["depth"], B, b["K"], 1, rle=(ptr(b["c"]), ptr(b["o"])), area_hint=ptr(b["ah"])) for b in ub]
    lines["rle_uniform_area_hint"] = lambda k: check(lib.la3d_fit_instances_ex(C.byref(rle_h[k % R])), "rle hint")
    lines["rle_frames_one_size_area_hint"] = lambda k: check(lib.la3d_fit_instances_frames(C.byref(fr_rle_h[k % R]), ptr(tab_d), B), "frames rle hint")
    lines["poly_frames_one_size_area_hint"] = lambda k: check(lib.la3d_fit_instances_frames(C.byref(fr_poly_h[k % R]), ptr(tab_d), B), "frames poly hint")
    lines["rle_frames_one_size"] = lambda k: check(lib.la3d_fit_instances_frames(C.byref(fr_rle[k % R]), ptr(tab_d), B), "frames rle")
    lines["poly_frames_one_size"] = lambda k: check(lib.la3d_fit_instances_frames(C.byref(fr_poly[k % R]), ptr(tab_d), B), "frames poly")
result["uniform_1024_us_per_call"] = alternate(lines)
torch.cuda.synchronize()
assert int((fu.status[0] == 0).sum()) == B, "a timed call left an unfitted instance"
del ub, rle_blocks, poly_blocks
torch.cuda.empty_cache()

# ---- (a) one mixed call against the calls grouped by size --------------------------------------------------------------------------
mixes = [coco_mix(77 + r) for r in range(R)]
grouped = [prepare_grouped(m) for m in mixes]
lines = {"grouped_by_size": lambda k: grouped[k % R][0]()}
if HAVE_FRAMES:
    mixed = [prepare_mixed(m) for m in mixes]
    lines["one_mixed_call"] = lambda k: mixed[k % R][0]()
times = alternate(lines)
torch.cuda.synchronize()
n_inst = [len(m["rle"]["img"]) + len(m["poly"]["img"]) for m in mixes]
info = dict(images=args.images, frame_sizes=len(set(mixes[0]["sizes"])), images_per_size=sorted((np.unique([f"{h}x{w}" for h, w in mixes[0]["sizes"]], return_counts=True)[1]).tolist(), reverse=True),
            instances=n_inst, grouped_calls_per_step=[len(g[1]) for g in grouped], mixed_calls_per_step=2)
if HAVE_FRAMES:
    # the two ways fit the same instances to the same statuses
    for (_, gcalls, _), (_, mcalls, _), m in zip(grouped, mixed, mixes):
        for kind, (a, f, Bm) in zip(("rle", "poly"), mcalls):
            st_m = f.status[0][:Bm].cpu().numpy()
            st_g = np.full(Bm, -1, np.int32)
            for ga, gf, gB, gk, sel in gcalls:
                if gk == kind:
                    st_g[sel] = gf.status[0][:gB].cpu().numpy()
            assert (st_m == st_g).all(), "the mixed call and the grouped calls disagree on a status"
    info["fitted_fraction"] = float(np.mean([float((f.status[0][:Bm] == 0).float().mean()) for _, mcalls, _ in mixed for _, f, Bm in mcalls]))
    info["mixed_over_grouped"] = times["one_mixed_call"]["median"] / times["grouped_by_size"]["median"]
    info["instances_per_second_mixed"] = float(np.mean(n_inst)) / (times["one_mixed_call"]["median"] * 1e-6)
info["instances_per_second_grouped"] = float(np.mean(n_inst)) / (times["grouped_by_size"]["median"] * 1e-6)
result["coco_mix_us_per_step"] = times
result["coco_mix"] = info
text = json.dumps(result, indent=1)
print(text)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
