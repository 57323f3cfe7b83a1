"""Measured lines of the bit-plane mask source: the same masks through the u8, the run-length and the bit-plane
entry, alternated in ONE process so that the run-to-run spread of every line is known.

    python profiles/bits/measure_bits.py --out profiles/bits/measure_bits.json            # this tree
    python profiles/bits/measure_bits.py --root <checkout of the parent commit> --out ...  # the parent's u8 / run-length lines

Inputs: BASELINE config 2's generator (bench.make_inputs: 480x640, private depth, RandomState(seed) rectangles), three resident
batches in rotation as bench.py does (seeds 1234, 1235, 1236), 5 warm-up + 20 timed steps per line, the lines alternated
A/B/C/A/B/C ``--reps`` times (default 6).  Every step is a pure enqueue of the C entry on prepared argument blocks; the 20 timed
steps stand between two HIP events.  A tree without the bit-plane entry (the parent commit) measures the u8 / run-length lines only.
Prints one JSON document; ``criteria`` holds the two comparisons the bit-plane change is held to:
  a) bits, un-grounded, per 1024 <= run lengths + the run-length line's own spread (max - min over the alternations)
  b) (by the reader, from two runs) u8 / run-length lines of this tree within their spread of the parent's."""
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
p.add_argument("--batches", default="1024,8192")
p.add_argument("--quick", action="store_true", help="B = 1024 only, two alternations (the profiler run)")
args = p.parse_args()
sys.path.insert(0, args.root)

import torch  # noqa: E402

import bench  # noqa: E402
from labelany3d_amd import _lib, batched  # noqa: E402
from labelany3d_amd._lib import check, lib  # noqa: E402

H, W, R = bench.H, bench.W, 3
HAVE_BITS = hasattr(lib, "la3d_fit_instances_bits")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731


def rect_rle(rects, B):
    """column-major run lengths of the rectangles bench.make_inputs draws (rows r0 .. r0+hh, columns c0 .. c0+ww)"""
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


def make_batches(B):
    out = []
    for r in range(R):
        depth, masks, K, npix, rects = bench.make_inputs(B, dev, 1234 + r)
        counts, offsets = rect_rle(rects, B)
        b = dict(depth=depth, masks=masks, K=K, counts=torch.as_tensor(counts, device=dev), offsets=torch.as_tensor(offsets, device=dev))
        rs = np.random.RandomState(99 + r)
        b["ground"] = torch.as_tensor(np.array([[0.02, -0.98, 0.1, 1.5]] * B) + 0.03 * rs.randn(B, 4), device=dev)
        if HAVE_BITS:
            b["bits"] = torch.empty((B, H * W // 32), dtype=torch.int32, device=dev)
            check(lib.la3d_pack_mask_bits(ptr(masks), H * W, B, H, W, W, ptr(b["bits"]), H * W // 32, None), "la3d_pack_mask_bits")
            b["bits2"] = torch.empty_like(b["bits"])
        out.append(b)
    dec = torch.empty_like(out[0]["masks"])   # the run lengths ARE the u8 planes
    check(lib.la3d_rle_decode(ptr(out[0]["counts"]), ptr(out[0]["offsets"]), B, H, W, ptr(dec), None), "la3d_rle_decode")
    torch.cuda.synchronize()
    assert torch.equal(dec, out[0]["masks"]), "rect_rle does not describe the rectangles"
    return out


def lines_for(B, batches):
    f = batched.InstanceFitter(B, H, W, dev)

    def block(b, grounded, **kw):
        return batched._fit_args(B, H, W, ptr(b["depth"]), B, ptr(b["K"]), 1, ptr(f.boxes[0]), ptr(f.status[0]), ptr(f.aux[0]),
                                 ptr(f.workspace[0]), C.c_void_p(st.cuda_stream), ground=ptr(b["ground"]) if grounded else None, **kw)
    lines = {}
    for grounded in (False, True):
        tag = "grounded" if grounded else "ungrounded"
        u8 = [block(b, grounded, mask=ptr(b["masks"])) for b in batches]
        rle = [block(b, grounded, rle=(ptr(b["counts"]), ptr(b["offsets"]))) for b in batches]
        lines[f"u8_{tag}"] = lambda k, a=u8: check(lib.la3d_fit_instances_ex(C.byref(a[k % R])), "u8")
        lines[f"rle_{tag}"] = lambda k, a=rle: check(lib.la3d_fit_instances_ex(C.byref(a[k % R])), "rle")
        if HAVE_BITS:
            bb = [block(b, grounded) for b in batches]
            lines[f"bits_{tag}"] = lambda k, a=bb: check(lib.la3d_fit_instances_bits(C.byref(a[k % R]), ptr(batches[k % R]["bits"]), H * W // 32, 0), "bits")
    if HAVE_BITS:
        bb2 = [block(b, False) for b in batches]

        def pack_fit(k):
            b = batches[k % R]
            check(lib.la3d_pack_mask_bits(ptr(b["masks"]), H * W, B, H, W, W, ptr(b["bits2"]), H * W // 32, C.c_void_p(st.cuda_stream)), "pack")
            check(lib.la3d_fit_instances_bits(C.byref(bb2[k % R]), ptr(b["bits2"]), H * W // 32, 0), "bits")
        lines["pack_plus_bits_ungrounded"] = pack_fit
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


result = dict(tree=args.root, have_bits=HAVE_BITS, build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0),
              steps=args.steps, warmup=args.warmup, fit_us_per_call={}, packers={})
reps = 2 if args.quick else args.reps
for B in ([1024] if args.quick else [int(x) for x in args.batches.split(",")]):
    batches = make_batches(B)
    lines, fitter = lines_for(B, batches)
    times = {k: [] for k in lines}
    for _ in range(reps):
        for name, fn in lines.items():
            times[name].append(time_line(fn))
    torch.cuda.synchronize()
    assert int((fitter.status[0] == 0).sum()) == B, "a timed call left an unfitted instance"
    result["fit_us_per_call"][str(B)] = {k: summarise(v) for k, v in times.items()}
    if B == 1024 and HAVE_BITS:
        # packers: bytes read + written per second, next to a plain device-to-device copy of the same number of bytes
        logits = [(b["masks"].to(torch.float16) - 0.5).contiguous() for b in batches]
        nw = H * W // 32
        by_mask, by_logit = B * (H * W + nw * 4), B * (H * W * 2 + nw * 4)
        cp_src = [torch.empty(by_mask // 2, dtype=torch.uint8, device=dev) for _ in range(R)]
        cp_dst = torch.empty(by_mask // 2, dtype=torch.uint8, device=dev)
        cl_src = [torch.empty(by_logit // 2, dtype=torch.uint8, device=dev) for _ in range(R)]
        cl_dst = torch.empty(by_logit // 2, dtype=torch.uint8, device=dev)
        sp = C.c_void_p(st.cuda_stream)
        pl = {
            "pack_mask_bits": (by_mask, lambda k: check(lib.la3d_pack_mask_bits(ptr(batches[k % R]["masks"]), H * W, B, H, W, W, ptr(batches[k % R]["bits2"]), nw, sp), "pack")),
            "copy_same_bytes_as_pack_mask_bits": (by_mask, lambda k: cp_dst.copy_(cp_src[k % R])),
            "pack_logits_bits_f16": (by_logit, lambda k: check(lib.la3d_pack_logits_bits(ptr(logits[k % R]), 1, H * W, 0.0, B, H, W, W, ptr(batches[k % R]["bits2"]), nw, sp), "logits")),
            "copy_same_bytes_as_pack_logits_bits": (by_logit, lambda k: cl_dst.copy_(cl_src[k % R])),
        }
        pt = {k: [] for k in pl}
        for _ in range(reps):
            for name, (nbytes, fn) in pl.items():
                pt[name].append(time_line(fn))
        for name, (nbytes, fn) in pl.items():
            s = summarise(pt[name])
            s["bytes_read_plus_written"] = nbytes
            s["GBps_median"] = nbytes / (s["median"] * 1e-6) / 1e9
            result["packers"][name] = s
        for b in batches:   # the device-packed planes are the planes the timed fits read
            assert torch.equal(b["bits"], b["bits2"])
        del logits, cp_src, cp_dst, cl_src, cl_dst
    del batches, lines, fitter
    torch.cuda.empty_cache()

l = result["fit_us_per_call"].get("1024", {})
if HAVE_BITS and l:
    rle, bits, u8 = l["rle_ungrounded"], l["bits_ungrounded"], l["u8_ungrounded"]
    result["criteria"] = {
        "a_bits_not_slower_than_rle_by_more_than_rle_spread": bool(bits["median"] <= rle["median"] + rle["spread"]),
        "a_bits_minus_rle_us": bits["median"] - rle["median"], "a_rle_spread_us": rle["spread"],
        "u8_over_bits": u8["median"] / bits["median"],
        "byte_model_MB_per_1024": {"u8": 449.0, "bits": 1024 * (H * W // 8) / 1e6 + 134.0},
    }
text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
