"""Measured lines of the 16-bit depth source (include/la3d.h "16-bit depth planes"): the same masks and the same
depth values through the float32 entry and through la3d_fit_instances_depth16, alternated in ONE process so that the run-to-run
spread of every line is known.

    python profiles/depth16/bench_depth16.py --out profiles/depth16/bench_depth16.json [--parent-lib <libla3d.so of the parent commit>]

Protocol of the round-6 bench: three resident input batches in rotation (seeds 1234 .. 1236), every line warmed up, 20 timed steps
between two HIP events, the lines alternated ``--reps`` times.  1024 instances of 640 x 480, private depth planes, two mask sets:
``config2`` (bench.make_inputs: rectangles of 8..300 x 8..330 px) and ``dense`` (rectangles of >= 50 % of the frame, where the depth
share of the traffic is largest).  Per mask source (u8 planes, bit planes, run lengths), everything pinned to the instance engine:
  a  the float32 call through the PARENT commit's library (``--parent-lib``: that commit built with LA3D_LIB=<path>; skipped if absent)
  b  the float32 call through this tree's library
  c  the float16 call and the uint16 call (1 mm units, zero = hole)
  d  what a caller does today: ``tensor.float()`` on the float16 planes, then a (b when there is no parent library)
The float32 planes ARE the up-converted float16 planes, so a / b / c_f16 fit the same values.  ``required_MB`` is the byte model of
VERDICT.md: mask bytes plus the 32 x 8-pixel depth tiles that hold a mask pixel, from the rectangles.  Prints one JSON document."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
p = argparse.ArgumentParser()
p.add_argument("--parent-lib", default=os.path.join(ROOT, "profiles", "depth16", "libla3d_parent.so"))
p.add_argument("--out", default=None)
p.add_argument("--reps", type=int, default=6)
p.add_argument("--steps", type=int, default=20)
p.add_argument("--warmup", type=int, default=5)
p.add_argument("--B", type=int, default=1024)
p.add_argument("--quick", action="store_true", help="config2 masks, 16-bit lines only, two alternations (the profiler run)")
args = p.parse_args()
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from labelany3d_amd import _lib, batched  # noqa: E402
from labelany3d_amd._lib import check, lib  # noqa: E402

H, W, R, B = bench.H, bench.W, 3, args.B
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()
sp = C.c_void_p(st.cuda_stream)
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
INSTANCE = (1, 0, 0)   # opt_engine = LA3D_ENGINE_INSTANCE

parent = None
if not args.quick and os.path.exists(args.parent_lib):
    parent = C.CDLL(args.parent_lib)
    parent.la3d_fit_instances_ex.argtypes = [C.POINTER(_lib.FitArgs)]
    parent.la3d_fit_instances_bits.argtypes = [C.POINTER(_lib.FitArgs), C.c_void_p, C.c_int64, C.c_int32]
    parent.la3d_build_info.restype = C.c_char_p


def rects_for(kind, seed):
    rs = np.random.RandomState(seed)
    if kind == "config2":   # bench.make_inputs' draw
        hh, ww = rs.randint(8, 301, B), rs.randint(8, 331, B)
    else:                    # >= 50 % of the frame: 340 x 460 = 156 400 of 307 200 px
        hh, ww = rs.randint(340, H + 1, B), rs.randint(460, W + 1, B)
    r0 = (rs.rand(B) * (H - hh + 1)).astype(np.int64)
    c0 = (rs.rand(B) * (W - ww + 1)).astype(np.int64)
    return r0, c0, hh, ww


def rect_rle(rects):
    r0, c0, hh, ww = rects
    counts, offsets = [], [0]
    for i in range(B):
        c = [int(c0[i]) * H + int(r0[i])]
        for j in range(int(ww[i])):
            c.append(int(hh[i]))
            c.append(H - int(hh[i]))
        c[-1] = H * W - sum(c[:-1])
        counts.extend(c)
        offsets.append(len(counts))
    return np.asarray(counts, np.int32), np.asarray(offsets, np.int64)


def tiles_px(rects):
    """pixels of the 32 x 8 depth tiles that hold a mask pixel, summed over the batch"""
    r0, c0, hh, ww = rects
    tx = -(-(c0 + ww) // 32) - c0 // 32
    ty = -(-(r0 + hh) // 8) - r0 // 8
    return int((tx * ty).sum()) * 256


def make_batches(kind):
    out = []
    for r in range(R):
        g = torch.Generator(device=dev)
        g.manual_seed(1234 + r)
        d = torch.empty((B, H, W), dtype=torch.float32, device=dev).uniform_(0.5, 10.0, generator=g)
        f16 = d.to(torch.float16)
        u16 = (d * 1000.0).round_().to(torch.int32).to(torch.int16).view(torch.uint16)   # millimetres, < 32768
        f32 = f16.float()
        del d
        rects = rects_for(kind, 1234 + r)
        r0, c0, hh, ww = rects
        t = lambda a: torch.as_tensor(a, device=dev).view(B, 1, 1)  # noqa: E731
        rows, cols = torch.arange(H, device=dev).view(1, H, 1), torch.arange(W, device=dev).view(1, 1, W)
        masks = ((rows >= t(r0)) & (rows < t(r0 + hh)) & (cols >= t(c0)) & (cols < t(c0 + ww))).to(torch.uint8).contiguous()
        counts, offsets = rect_rle(rects)
        b = dict(f32=f32, f16=f16, u16=u16, masks=masks, counts=torch.as_tensor(counts, device=dev), offsets=torch.as_tensor(offsets, device=dev),
                 K=torch.tensor(bench.K640, dtype=torch.float64, device=dev), rects=rects, rle_bytes=int(counts.nbytes + offsets.nbytes))
        b["bits"] = torch.empty((B, H * W // 32), dtype=torch.int32, device=dev)
        check(lib.la3d_pack_mask_bits(ptr(masks), H * W, B, H, W, W, ptr(b["bits"]), H * W // 32, None), "la3d_pack_mask_bits")
        out.append(b)
    torch.cuda.synchronize()
    return out


def lines_for(batches):
    f = batched.InstanceFitter(B, H, W, dev)
    nw = H * W // 32

    def block(b, depth, **kw):
        return batched._fit_args(B, H, W, depth, B, ptr(b["K"]), 1, ptr(f.boxes[0]), ptr(f.status[0]), ptr(f.aux[0]), ptr(f.workspace[0]), sp,
                                 opts=INSTANCE, **kw)

    def call(L, a, b, src):
        if src == "bits":
            check(L.la3d_fit_instances_bits(C.byref(a), ptr(b["bits"]), nw, 0), "bits")
        else:
            check(L.la3d_fit_instances_ex(C.byref(a)), src)

    def call16(a, b, src):
        check(lib.la3d_fit_instances_depth16(C.byref(a), C.byref(a.d16), ptr(b["bits"]) if src == "bits" else None, nw if src == "bits" else 0, 0), src)

    lines = {}
    for src in ("u8", "bits", "rle"):
        mk = {"u8": lambda b: dict(mask=ptr(b["masks"])), "bits": lambda b: {}, "rle": lambda b: dict(rle=(ptr(b["counts"]), ptr(b["offsets"])))}[src]
        a32 = [block(b, ptr(b["f32"]), **mk(b)) for b in batches]
        af16 = [block(b, batched.Depth16(b["f16"]), **mk(b)) for b in batches]
        au16 = [block(b, batched.Depth16(b["u16"], 0.001, True), **mk(b)) for b in batches]
        if not args.quick:
            if parent is not None:
                lines[f"{src}.a_parent_f32"] = lambda k, a=a32, s=src: call(parent, a[k % R], batches[k % R], s)
            lines[f"{src}.b_branch_f32"] = lambda k, a=a32, s=src: call(lib, a[k % R], batches[k % R], s)
        lines[f"{src}.c_f16"] = lambda k, a=af16, s=src: call16(a[k % R], batches[k % R], s)
        lines[f"{src}.c_u16"] = lambda k, a=au16, s=src: call16(a[k % R], batches[k % R], s)
        if not args.quick:
            base = parent if parent is not None else lib

            def today(k, s=src, mk=mk):
                b = batches[k % R]
                up = b["f16"].float()   # what a caller does today (a new float32 copy: 2 B read + 4 B written per pixel)
                call(base, block(b, ptr(up), **mk(b)), b, s)
            lines[f"{src}.d_float_plus_{'a' if parent is not None else 'b'}"] = today
    return lines, f


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


result = dict(build_info=lib.la3d_build_info().decode(), parent_build_info=parent.la3d_build_info().decode() if parent is not None else None,
              device=torch.cuda.get_device_name(0), B=B, steps=args.steps, warmup=args.warmup, us_per_call={}, required_MB={}, criteria={})
reps = 2 if args.quick else args.reps
for kind in (["config2"] if args.quick else ["config2", "dense"]):
    batches = make_batches(kind)
    lines, fitter = lines_for(batches)
    times = {k: [] for k in lines}
    for _ in range(reps):
        for name, fn in lines.items():
            times[name].append(time_line(fn))
    torch.cuda.synchronize()
    assert int((fitter.status[0] == 0).sum()) == B, "a timed call left an unfitted instance"
    # the 16-bit calls fit what the float32 call fits: float16 bit for bit on the up-converted planes
    b = batches[0]
    lines["u8.c_f16"](0); torch.cuda.synchronize(); got = fitter.boxes[0].clone()
    (lines.get("u8.b_branch_f32") or lines["u8.c_f16"])(0); torch.cuda.synchronize()
    assert torch.allclose(got, fitter.boxes[0], rtol=1e-12, atol=1e-12), "float16 and float32 records differ"
    res = {k: summarise(v) for k, v in times.items()}
    result["us_per_call"][kind] = res
    px = float(np.mean([tiles_px(b["rects"]) for b in batches]))
    mask_bytes = {"u8": B * H * W, "bits": B * H * W // 8, "rle": float(np.mean([b["rle_bytes"] for b in batches]))}
    result["required_MB"][kind] = {src: {"f32": (mask_bytes[src] + 4 * px) / 1e6, "16bit": (mask_bytes[src] + 2 * px) / 1e6,
                                         "today_f16_to_f32_pass": B * H * W * 6 / 1e6} for src in mask_bytes}
    if not args.quick:
        crit = {}
        for src in ("u8", "bits", "rle"):
            bl, d = res[f"{src}.b_branch_f32"], res[[k for k in res if k.startswith(f"{src}.d_")][0]]
            spread = max(bl["spread"], res.get(f"{src}.a_parent_f32", bl)["spread"])
            for c in ("c_f16", "c_u16"):
                cc = res[f"{src}.{c}"]
                crit[f"{src}.{c}"] = dict(faster_than_d=bool(cc["median"] < d["median"]), minus_b_us=cc["median"] - bl["median"],
                                          spread_us=spread, not_slower_than_b_by_more_than_spread=bool(cc["median"] <= bl["median"] + spread))
            if parent is not None:
                crit[f"{src}.b_minus_a_us"] = bl["median"] - res[f"{src}.a_parent_f32"]["median"]
        result["criteria"][kind] = crit
    del batches, lines, fitter
    torch.cuda.empty_cache()

text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
