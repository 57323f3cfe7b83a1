"""Measured lines of the frames call on 16-bit depth planes and of ``ScenePipeline(depth_dtype=...)``, every
comparison alternated in ONE process so that the run-to-run spread of each line is known.

    python profiles/frames16/measure_frames16.py --out profiles/frames16/measure_frames16.json     # this tree
    python profiles/frames16/measure_frames16.py --root <checkout of the parent commit> --device-only --out ...   # the parent's float32 line

(a) device: the COCO-like mix of profiles/frames/measure_frames.py (256 images over 18 frame sizes, ~7 instances per image, polygons
    75 % / run lengths 25 %, the fused filter on, annotation areas as ``area_hint``), ONE frames call per annotation kind from float32
    planes, from float16 planes, from uint16 (millimetre) planes, and "what a caller of 16-bit planes does today": the up-conversion
    of the ragged 16-bit buffer (``la3d_unpack_depth16``) followed by the float32 frames call.  Pure enqueues of prepared argument
    blocks on resident inputs.  Three resident batches in rotation, 5 warm-up + 20 timed steps per line between two HIP events, the
    lines alternated ``--reps`` times (default 6); median, min, max of every line.
(b) host to records: ``ScenePipeline`` over ``--scenes`` host-resident synthetic scenes (``synthetic_scenes``; ``--distinct`` different
    ones, repeated) of 640 x 480 and of 500 x 375 in the uniform mode and of four sizes in the mixed mode, float32 against uint16: images/s, bytes
    uploaded per image, the pack / H2D / fit / D2H split of ``timings`` and the fraction of the pinned host-to-device rate measured in
    the same run."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

p = argparse.ArgumentParser()
p.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
p.add_argument("--out", default=None)
p.add_argument("--reps", type=int, default=6)
p.add_argument("--steps", type=int, default=20)
p.add_argument("--warmup", type=int, default=5)
p.add_argument("--images", type=int, default=256)
p.add_argument("--scenes", type=int, default=2048)
p.add_argument("--distinct", type=int, default=128)
p.add_argument("--device-only", action="store_true")
p.add_argument("--host-only", action="store_true")
args = p.parse_args()
sys.path.insert(0, args.root)

import torch  # noqa: E402

from labelany3d_amd import batched, masks  # noqa: E402
from labelany3d_amd._lib import check, lib  # noqa: E402
from labelany3d_amd import _lib  # noqa: E402

R = 3
HAVE16 = hasattr(lib, "la3d_fit_instances_frames_depth16")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
FLT = {"boundary_threshold": 10, "scale_threshold": 100}
SCALE = 0.001
COCO_SIZES = [(480, 640), (640, 480), (427, 640), (640, 427), (426, 640), (428, 640), (375, 500), (500, 375), (333, 500), (425, 640),
              (480, 480), (640, 640), (360, 640), (500, 333), (612, 612), (424, 640), (334, 500), (512, 640)]


def quantise(d32, dtype):
    """plain NumPy, the rules of tests/depth16_cases.py::quantise"""
    if dtype == "f16":
        return d32.astype(np.float16)
    q = np.rint(d32 / np.float32(SCALE))
    return np.where(np.isfinite(d32) & (d32 > 0), np.minimum(q, np.float32(65535)), np.float32(0)).astype(np.uint16)


def rle_of(m):
    flat = m.ravel(order="F")
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return ([0] + counts) if flat[0] else counts


def coco_mix(seed):
    """the mix of profiles/frames/measure_frames.py: images, their sizes, and the annotations of both kinds with image index and area"""
    rs = np.random.RandomState(seed)
    share = 1.0 / np.arange(1, len(COCO_SIZES) + 1)
    share /= share.sum()
    n = np.maximum(1, np.round(share * args.images).astype(int))
    n[0] += args.images - n.sum()
    sizes = [s for s, k in zip(COCO_SIZES, n) for _ in range(k)]
    sizes = [sizes[i] for i in rs.permutation(len(sizes))]
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


def prepare(mix, dtype):
    """one frames call per annotation kind on float32 (dtype None), float16 or uint16 planes; "convert": uint16 planes, up-converted
    into a float32 buffer of the same layout before the float32 calls"""
    convert = dtype == "convert"
    src = None if dtype is None else ("u16" if convert else dtype)
    if src is None:
        pf = masks.pack_frames(mix["depth"], device=dev)
        planes = pf.depth
    else:
        pf = masks.pack_frames([quantise(d, src) for d in mix["depth"]], device=dev, dtype=src, scale=SCALE)
        planes = pf.data
    keep = [pf]
    blk = unpack = None
    if src is not None:
        u16 = src == "u16"
        blk = _lib.Depth16Block(struct_size=C.sizeof(_lib.Depth16Block), dtype=_lib.DTYPE_U16 if u16 else _lib.DTYPE_F16, planes=planes.data_ptr(),
                                plane_stride=0, scale=SCALE if u16 else 1.0, flags=_lib.DEPTH_ZERO_IS_HOLE if u16 else 0)
    if convert:   # (every pitch is a multiple of 32: the ragged buffer is one dense plane of rows of 32 words)
        f32 = torch.empty(planes.numel(), dtype=torch.float32, device=dev)
        rows = planes.numel() // 32
        keep.append(f32)
        unpack = lambda: check(lib.la3d_unpack_depth16(C.byref(blk), 1, rows, 32, 32, ptr(f32), C.c_void_p(st.cuda_stream)), "unpack")  # noqa: E731
        planes = f32
    K = up(mix["K"])
    keep.append(K)
    calls = []
    for kind in ("rle", "poly"):
        g = mix[kind]
        B = len(g["img"])
        f = batched.InstanceFitter(B, pf.H, pf.W, dev)
        ii, ah, stats = up(np.asarray(g["img"], np.int32)), up(np.asarray(g["area"], np.int32)), torch.zeros((B, 4), dtype=torch.int32, device=dev)
        if kind == "rle":
            c, o = up(np.asarray(g["counts"], np.int32)), up(np.asarray(g["offsets"], np.int64))
            src_kw = dict(rle=(ptr(c), ptr(o)))
            keep += [c, o]
        else:
            xy, ro, ir = up(np.concatenate(g["xy"])), up(np.asarray(g["ring"], np.int64)), up(np.asarray(g["inst"], np.int64))
            src_kw = dict(poly=(ptr(xy), ptr(ro), ptr(ir)))
            keep += [xy, ro, ir]
        direct16 = src is not None and not convert
        a = batched._fit_args(B, pf.H, pf.W, None if direct16 else ptr(planes), 1, ptr(K), len(K), ptr(f.boxes[0]), ptr(f.status[0]), ptr(f.aux[0]),
                              ptr(f.workspace[0]), C.c_void_p(st.cuda_stream), image_index=ptr(ii), area_hint=ptr(ah), filter=FLT, stats=ptr(stats), **src_kw)
        keep += [f, ii, ah, stats]
        calls.append((a, f, B))
    table, P = pf.table, len(mix["sizes"])

    def run():
        if unpack is not None:
            unpack()
        for a, _, _ in calls:
            if src is not None and not convert:
                check(lib.la3d_fit_instances_frames_depth16(C.byref(a), C.byref(blk), ptr(table), P), "frames16")
            else:
                check(lib.la3d_fit_instances_frames(C.byref(a), ptr(table), P), "frames")
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


result = dict(tree=os.path.relpath(args.root), have_frames16=HAVE16, build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0),
              steps=args.steps, warmup=args.warmup, reps=args.reps)

if not args.host_only:
    mixes = [coco_mix(77 + r) for r in range(R)]
    prepared = {"float32": [prepare(m, None) for m in mixes]}
    if HAVE16:
        prepared["float16"] = [prepare(m, "f16") for m in mixes]
        prepared["uint16"] = [prepare(m, "u16") for m in mixes]
        prepared["uint16_converted_first"] = [prepare(m, "convert") for m in mixes]
    lines = {name: (lambda k, q=q: q[k % R][0]()) for name, q in prepared.items()}
    times = alternate(lines)
    torch.cuda.synchronize()
    n_inst = [len(m["rle"]["img"]) + len(m["poly"]["img"]) for m in mixes]
    info = dict(images=args.images, frame_sizes=len(set(mixes[0]["sizes"])), instances=n_inst,
                depth_bytes_float32=int(prepared["float32"][0][2][0].depth.numel() * 4))
    if HAVE16:
        info["depth_bytes_16bit"] = int(prepared["uint16"][0][2][0].data.numel() * 2)
        # the converted-first line fits what the direct uint16 line fits: same statuses, same records
        same = True
        for (_, ca, _), (_, cb, _) in zip(prepared["uint16"], prepared["uint16_converted_first"]):
            for (_, fa, B), (_, fb, _) in zip(ca, cb):
                same = same and torch.equal(fa.status[0][:B], fb.status[0][:B]) and torch.equal(torch.nan_to_num(fa.boxes[0][:B]), torch.nan_to_num(fb.boxes[0][:B]))
        info["direct_equals_converted_first"] = bool(same)
        info["fitted_fraction"] = float(np.mean([float((f.status[0][:B] == 0).float().mean()) for _, calls, _ in prepared["uint16"] for _, f, B in calls]))
    result["coco_mix_us_per_step"] = times
    result["coco_mix"] = info
    del prepared
    torch.cuda.empty_cache()

if not args.device_only and HAVE16:
    from labelany3d_amd.fit_scenes import ScenePipeline, synthetic_scenes

    # the pinned host-to-device rate of this run: 256 MiB, five copies
    pin = torch.empty(256 << 20, dtype=torch.uint8, pin_memory=True)
    dst = torch.empty_like(pin, device=dev)
    dst.copy_(pin, non_blocking=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(st)
    for _ in range(5):
        dst.copy_(pin, non_blocking=True)
    e1.record(st)
    torch.cuda.synchronize()
    h2d_rate = 5 * pin.numel() / (e0.elapsed_time(e1) * 1e-3)
    del pin, dst
    result["pinned_h2d_bytes_per_s"] = h2d_rate

    def scene_set(sizes):
        """(float32 scenes, the same scenes with uint16 planes): --distinct different ones, repeated to --scenes"""
        per = max(1, args.distinct // len(sizes))
        base = []
        for k, (h, w) in enumerate(sizes):
            sc, _ = synthetic_scenes(per, seed=300 + k, H=h, W=w)
            base.append(sc)
        base = [s for group in zip(*base) for s in group]         # interleaved: the sizes arrive mixed
        base16 = [dict(sc, depth=quantise(sc["depth"], "u16")) for sc in base]
        reps = (args.scenes + len(base) - 1) // len(base)
        expand = lambda b: [dict(sc, name=f"{r}-{sc['name']}-{sc['height']}x{sc['width']}") for r in range(reps) for sc in b][:args.scenes]  # noqa: E731
        return expand(base), expand(base16)

    def run_pipe(scenes, **kw):
        t = {}
        pipe = ScenePipeline(device=dev, write=False, timings=t, **kw)
        t0 = time.perf_counter()
        boxes = sum(len(recs) for _, recs in pipe.run(scenes))
        wall = time.perf_counter() - t0
        n = len(scenes)
        return dict(images_per_s=n / wall, wall_s=wall, boxes=boxes, h2d_bytes_per_image=t["h2d_bytes"] / n,
                    split_s={k: t[k] for k in ("load_s", "pack_s", "h2d_s", "fit_s", "write_s")},
                    fraction_of_pinned_h2d_rate=(t["h2d_bytes"] / wall) / h2d_rate)

    host = {}
    # (500 x 375: a width that is no multiple of 32 - the uniform 16-bit mode uploads such planes at the padded pitch, row by row)
    for label, sizes, kw in (("uniform_640x480", [(480, 640)], {}), ("uniform_500x375", [(375, 500)], {}), ("mixed_four_sizes", [(480, 640), (427, 640), (375, 500), (500, 333)], dict(mixed_frames=True))):
        f32, u16 = scene_set(sizes)
        runs = {"float32": [], "uint16": []}
        for _ in range(3):                                      # alternated; the first pair warms the pinned buffers up and is dropped
            runs["float32"].append(run_pipe(f32, **kw))
            runs["uint16"].append(run_pipe(u16, depth_dtype="u16", depth_scale=SCALE, **kw))
        host[label] = {k: dict(runs=v[1:], images_per_s_median=float(np.median([r["images_per_s"] for r in v[1:]]))) for k, v in runs.items()}
        assert runs["float32"][-1]["boxes"] > 0 and runs["uint16"][-1]["boxes"] > 0
    result["scene_pipeline"] = dict(scenes=args.scenes, distinct=args.distinct, lines=host)

text = json.dumps(result, indent=1)
print(text)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
