"""Measured lines of the opening on bit planes (include/la3d.h "morphology on bit planes"; RESULTS.md beside this file): resident
``MaskBits`` of 640 x 480 frames -> the opened planes of the x4 upscale (k = 7, the crop stage's gate) with their areas and rectangles,
against the two routes a caller had before, alternated in ONE process so that the spread of every line is known (the protocol of
profiles/crop_bits/bench_crop_bits.py).

    python profiles/open_bits/bench_open_bits.py --out profiles/open_bits/bench_open_bits.json

Inputs: B = 1 / 16 / 256 planes (s = 4) and B = 1024 planes (s = 1), each the union of three rectangles or ellipses XORed with 2 % salt
noise; three batches in rotation.
  new.open      open_bits(k = 7, upscale = s, out =, return_stats = True): the kernel pair, planes and statistics, nothing leaves the device
  new.select    select_crops: new.open + the read-back of the statistics + crop_params on the host (host clock, ends synchronised)
  new.stats     the statistics-only call (out_bits = NULL) through the C entry
  b.total       device route of the parent: unpack_mask_bits, repeat_interleave x s on both axes, erosion and dilation by max_pool2d on
                -mask / +mask (float16; the erosion pads -mask with 0, so that pixels outside count as unset, the dilation with
                -inf), pack_mask_bits, torch reductions for area and rectangle
  a.total       host route of the parent (B <= 16 only: SciPy takes a quarter of a second per upscaled plane): unpack, copy to the
                host, np.repeat, scipy.ndimage.binary_opening, the rectangle in NumPy (host clock)
  pack          pack_mask_bits on resident (B, 480, 640) u8 planes: the packer whose byte rate new.open is held against
``model_MB`` = the bytes a line must move: new.open B * (H * W / 8 + s * H * s * W / 8), pack B * (H * W + H * W / 8); ``model_GBps`` =
that over the median time.  Every line is warmed up and timed over ``steps`` calls - device lines between two HIP events with the
host's clock beside them (``host_us``), host lines on the host's clock around a loop that ends in a synchronise -, ``steps`` raised
until a run lasts ``--min-ms``, the lines alternated ``--reps`` times.  Before anything is timed the routes are compared bit for bit.
Prints one JSON document."""
import argparse
import ctypes as C
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
p.add_argument("--cases", default="1:4,16:4,256:4,1024:1", help="B:upscale, comma separated")
p.add_argument("--min-ms", type=float, default=60.0, help="a timed run lasts at least this long")
p.add_argument("--host-max", type=int, default=16, help="largest batch the host route is run at")
args = p.parse_args()
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import labelany3d_amd as la  # noqa: E402
from labelany3d_amd._lib import lib  # noqa: E402

H, W, K, R = 480, 640, 7, 3
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()


def make_batch(B, seed):
    """B planes: 32 seeded shapes in rotation, each plane with salt noise of its own"""
    rs = np.random.RandomState(seed)
    vv, uu = np.mgrid[0:H, 0:W]
    shapes = np.zeros((min(B, 32), H, W), bool)
    for b in range(len(shapes)):
        for _ in range(3):
            cy, cx, hy, hx = rs.randint(0, H), rs.randint(0, W), rs.randint(8, H // 3), rs.randint(8, W // 3)
            if rs.rand() < 0.5:
                shapes[b] |= (np.abs(vv - cy) <= hy) & (np.abs(uu - cx) <= hx)
            else:
                shapes[b] |= ((vv - cy) / float(hy)) ** 2 + ((uu - cx) / float(hx)) ** 2 <= 1.0
    noise = torch.rand((B, H, W), generator=torch.Generator().manual_seed(seed)) < 0.02
    return shapes[np.arange(B) % len(shapes)] ^ noise.numpy()


def rects_torch(m):
    """(B, H, W) bool on the device -> (B, 5) area, x, y, w, h by torch reductions"""
    rows, cols = m.any(2), m.any(1)
    y0, x0 = rows.int().argmax(1), cols.int().argmax(1)
    y1, x1 = m.shape[1] - 1 - rows.flip(1).int().argmax(1), m.shape[2] - 1 - cols.flip(1).int().argmax(1)
    area = m.sum((1, 2))
    some = area > 0
    return torch.stack([area, x0 * some, y0 * some, (x1 - x0 + 1) * some, (y1 - y0 + 1) * some], 1).int()


def route_b(bits, s, out):
    m = la.unpack_mask_bits(bits)
    if s > 1:
        m = m.repeat_interleave(s, 1).repeat_interleave(s, 2)
    x = m.to(torch.float16)[:, None]
    r = K // 2
    e = -F.max_pool2d(F.pad(-x, (r, r, r, r), value=0.0), K, 1)          # erosion: outside counts as unset
    d = F.max_pool2d(e, K, 1, padding=r)                                  # dilation: the -inf padding never wins
    o = d[:, 0] > 0.5
    return la.pack_mask_bits(o, out=out), rects_torch(o)


def route_a(bits, s):
    from scipy.ndimage import binary_opening

    m = la.unpack_mask_bits(bits).cpu().numpy()
    outs, stats = [], []
    for one in m:
        o = binary_opening(np.repeat(np.repeat(one, s, 0), s, 1), np.ones((K, K)))
        rows, cols = np.flatnonzero(o.any(1)), np.flatnonzero(o.any(0))
        stats.append([int(o.sum()), cols[0], rows[0], cols[-1] - cols[0] + 1, rows[-1] - rows[0] + 1] if len(rows) else [0] * 5)
        outs.append(o)
    return outs, np.array(stats, np.int32)


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


result = dict(build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0), frame=[H, W], k=K, reps=args.reps, lines={})
for case in args.cases.split(","):
    B, s = (int(x) for x in case.split(":"))
    Ho, Wo = s * H, s * W
    bs = []
    for r in range(R):
        u8 = torch.as_tensor(make_batch(B, 1900 + r).view(np.uint8), device=dev)
        bs.append(dict(u8=u8, bits=la.pack_mask_bits(u8), out=torch.empty((B, Ho * Wo // 32), dtype=torch.int32, device=dev),
                       out_b=torch.empty((B, Ho * Wo // 32), dtype=torch.int32, device=dev),
                       stats=torch.empty((B, 5), dtype=torch.int32, device=dev)))
    ws = torch.empty(max(int(lib.la3d_open_bits_workspace_bytes(B, H, s)) // 4, 1), dtype=torch.int32, device=dev)
    # the routes give the same planes and statistics, bit for bit
    b0 = bs[0]
    new, new_stats = la.open_bits(b0["bits"], k=K, upscale=s, return_stats=True)
    rb, rb_stats = route_b(b0["bits"], s, b0["out_b"])
    assert torch.equal(new.bits, rb.bits) and torch.equal(new_stats, rb_stats) and int(new_stats[:, 0].sum()) > 0
    if B <= args.host_max:
        ra, ra_stats = route_a(b0["bits"], s)
        assert np.array_equal(new_stats.cpu().numpy(), ra_stats)
        assert torch.equal(la.pack_mask_bits(torch.as_tensor(np.stack(ra).view(np.uint8), device=dev)).bits, new.bits)

    def stats_only(k):
        b = bs[k % R]
        rc = lib.la3d_open_bits(C.c_void_p(b["bits"].bits.data_ptr()), b["bits"].bits.stride(0) if B > 1 else b["bits"].bits.shape[1], B, H, W, W, K, s,
                                None, 0, 0, C.c_void_p(b["stats"].data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(st.cuda_stream))
        assert rc == 0

    stats_only(0)
    assert torch.equal(bs[0]["stats"], new_stats)
    lines = {
        "new.open": (lambda k: la.open_bits(bs[k % R]["bits"], k=K, upscale=s, out=bs[k % R]["out"], return_stats=True), time_device),
        "new.stats": (stats_only, time_device),
        "new.select": (lambda k: la.select_crops(bs[k % R]["bits"], k=K, upscale=s), time_host),
        "b.total": (lambda k: route_b(bs[k % R]["bits"], s, bs[k % R]["out_b"]), time_device),
        "pack": (lambda k: la.pack_mask_bits(bs[k % R]["u8"], out=bs[k % R]["out"][:, :H * W // 32]), time_device),
    }
    if B <= args.host_max:
        lines["a.total"] = (lambda k: route_a(bs[k % R]["bits"], s), time_host)
    nsteps = {}
    for name, (fn, timer) in lines.items():   # a run lasts at least --min-ms: from a pilot
        if name == "a.total":
            nsteps[name] = 1 if B > 1 else 2
            continue
        ev, host = timer(fn, 2, 1)
        nsteps[name] = max(2, int(np.ceil(args.min_ms * 1e3 / max(ev, host, 1e-3))))
    times = {k: [] for k in lines}
    for _ in range(args.reps):
        for name, (fn, timer) in lines.items():
            times[name].append(timer(fn, nsteps[name], 0 if name == "a.total" else max(nsteps[name] // 10, 1)))
    res = {k: summarise(v) for k, v in times.items()}
    mb_new, mb_pack = B * (H * W // 8 + Ho * Wo // 8), B * (H * W + H * W // 8)
    res["new.open"].update(model_MB=mb_new / 1e6, model_GBps=mb_new / (res["new.open"]["median"] * 1e-6) / 1e9,
                           b_total_over_new=res["b.total"]["median"] / res["new.open"]["median"])
    res["pack"].update(model_MB=mb_pack / 1e6, model_GBps=mb_pack / (res["pack"]["median"] * 1e-6) / 1e9)
    if "a.total" in res:
        res["new.select"].update(a_total_over_new=res["a.total"]["median"] / res["new.select"]["median"])
    res["steps"] = nsteps
    result["lines"][f"B={B},s={s}"] = res
    print(f"B={B} s={s}", {k: round(v["median"], 1) for k, v in res.items() if isinstance(v, dict) and "median" in v}, flush=True)
    del bs, b0, new, new_stats, rb, rb_stats, lines, ws
    torch.cuda.empty_cache()

text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
