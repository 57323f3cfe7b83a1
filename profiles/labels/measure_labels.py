"""Measured lines of the label-map mask source: the same instances through today's route (expand the label
map into u8 planes in torch, then the u8 fit) and through the label-map route, alternated in ONE process so that the run-to-run
spread of every line is known.

    python profiles/labels/measure_labels.py --out profiles/labels/measure_labels.json            # this tree
    python profiles/labels/measure_labels.py --root <checkout of the parent commit> --out ...      # the parent's lines (a) and (c)

Workload: the config-3 shape - 640 x 480, one shared depth plane per image, 7 instances per image (blocky label maps: rectangles of
log-uniform area 400 .. 100k px painted over an unlabeled background, later ones over earlier ones), B = 1022 (146 images) and
B = 8190 (1170 images).  Three resident input sets in rotation, 5 warm-up + 20 timed steps per line between two HIP events, the
lines alternated ``--reps`` times (default 6); the spread of a line is max - min over the alternations.

Lines (us per call):
  a_expand_then_u8     torch ``labels[image_index] == ids[:, None, None]`` -> (B,H,W) u8, then ``fit_instances(..., image_index=)``
  a_c_*                the same on the C entry (la3d_fit_instances_ex on a prepared block): no wrapper, no allocation but torch's
  b_pack_<dtype>       la3d_pack_label_bits alone, U8 / U16 / I32 / RGB8 label maps
  c_bits               la3d_fit_instances_bits on already packed planes (prepared block)
  d_labels             ``fit_instances_labels`` end to end (U8 label maps)
  d_c_*                la3d_pack_label_bits + la3d_fit_instances_bits (image_index, area_hint = the packer's areas) on prepared blocks
A tree without the label-map entry (the parent commit) measures (a) and (c) only.  ``criteria``: d <= a by more than a's spread;
for (b) the achieved bytes / s over the required bytes (P*H*W*s label bytes + B*nwords*4 plane bytes) beside the pure-reader rate of
the same run (la3d_mask_counts over the U8 label planes, as bench.py measures its stream ceiling)."""
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
p.add_argument("--images", default="146,1170")
p.add_argument("--quick", action="store_true", help="146 images only, two alternations (the profiler run)")
args = p.parse_args()
sys.path.insert(0, args.root)

import torch  # noqa: E402

import bench  # noqa: E402
import labelany3d_amd as la  # noqa: E402
from labelany3d_amd import _lib, batched  # noqa: E402
from labelany3d_amd._lib import check, lib  # noqa: E402

H, W, R, PER = bench.H, bench.W, 3, 7
NW = H * W // 32
HAVE_LABELS = hasattr(lib, "la3d_pack_label_bits")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()
sp = C.c_void_p(st.cuda_stream)
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731


def make_set(P, seed):
    """one resident input set: depth (P,H,W), U8 label maps with ids 1 .. 7 over background 0, the (image, id) rows"""
    rs = np.random.RandomState(seed)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    depth = torch.empty((P, H, W), dtype=torch.float32, device=dev).uniform_(0.5, 10.0, generator=g)
    labels = torch.zeros((P, H, W), dtype=torch.uint8, device=dev)
    rows = torch.arange(H, device=dev).view(1, H, 1)
    cols = torch.arange(W, device=dev).view(1, 1, W)
    for k in range(1, PER + 1):
        area = np.exp(rs.uniform(np.log(400), np.log(100000), P))
        asp = np.exp(rs.uniform(-0.7, 0.7, P))
        hh = np.clip(np.sqrt(area * asp), 8, H).astype(np.int64)
        ww = np.clip(area / hh, 8, W).astype(np.int64)
        r0 = (rs.rand(P) * (H - hh + 1)).astype(np.int64)
        c0 = (rs.rand(P) * (W - ww + 1)).astype(np.int64)
        for a in range(0, P, 256):
            t = lambda v: torch.as_tensor(v[a:a + 256], device=dev).view(-1, 1, 1)  # noqa: E731
            inside = (rows >= t(r0)) & (rows < t(r0 + hh)) & (cols >= t(c0)) & (cols < t(c0 + ww))
            labels[a:a + 256][inside] = k
    B = P * PER
    ids = torch.arange(1, PER + 1, dtype=torch.int32, device=dev).repeat(P)
    ii = torch.arange(P, dtype=torch.int32, device=dev).repeat_interleave(PER)
    off = torch.arange(0, B + 1, PER, dtype=torch.int32, device=dev)
    K = torch.tensor(bench.K640, dtype=torch.float64, device=dev).expand(P, 3, 3).contiguous()
    s = dict(depth=depth, labels=labels, ids=ids, ii=ii, ii64=ii.long(), off=off, K=K, idv=ids.to(torch.uint8).view(-1, 1, 1),
             ids_list=[list(range(1, PER + 1))] * P)
    # planes packed WITHOUT the code under test: torch comparison + the u8 packer (present in the parent)
    s["bits"] = torch.empty((B, NW), dtype=torch.int32, device=dev)
    for a in range(0, B, 1024):
        m = (labels[s["ii64"][a:a + 1024]] == s["idv"][a:a + 1024]).view(torch.uint8)
        check(lib.la3d_pack_mask_bits(ptr(m), H * W, m.shape[0], H, W, W, ptr(s["bits"][a:a + 1024]), NW, sp), "la3d_pack_mask_bits")
    torch.cuda.synchronize()
    return s


def lines_for(P, sets):
    B = P * PER
    f = batched.InstanceFitter(B, H, W, dev)

    def block(s, **kw):
        return batched._fit_args(B, H, W, ptr(s["depth"]), P, ptr(s["K"]), P, ptr(f.boxes[0]), ptr(f.status[0]), ptr(f.aux[0]),
                                 ptr(f.workspace[0]), sp, image_index=ptr(s["ii"]), **kw)
    lines = {}

    def a_py(k):
        s = sets[k % R]
        la.fit_instances(s["depth"], s["labels"][s["ii64"]] == s["idv"], s["K"], image_index=s["ii"])
    lines["a_expand_then_u8"] = a_py
    blocks_a = [block(s) for s in sets]

    def a_c(k):
        s, a = sets[k % R], blocks_a[k % R]
        m = s["labels"][s["ii64"]] == s["idv"]
        a.mask = m.data_ptr()
        check(lib.la3d_fit_instances_ex(C.byref(a)), "u8")
    lines["a_c_expand_then_u8"] = a_c
    blocks_c = [block(s) for s in sets]
    lines["c_bits"] = lambda k: check(lib.la3d_fit_instances_bits(C.byref(blocks_c[k % R]), ptr(sets[k % R]["bits"]), NW, 0), "bits")
    packs = {}
    if HAVE_LABELS:
        bits2 = torch.empty((B, NW), dtype=torch.int32, device=dev)
        area = torch.empty(B, dtype=torch.int32, device=dev)
        for s in sets:
            s["u16"] = s["labels"].to(torch.int16)
            s["i32"] = s["labels"].to(torch.int32)
            s["rgb8"] = torch.stack([s["labels"], torch.zeros_like(s["labels"]), torch.zeros_like(s["labels"])], dim=-1).contiguous()

        def pack(k, key="labels", code=_lib.LABEL_U8):
            s = sets[k % R]
            check(lib.la3d_pack_label_bits(ptr(s[key]), code, H * W, P, H, W, W, ptr(s["off"]), ptr(s["ids"]), B, ptr(bits2), NW, ptr(area), sp),
                  "la3d_pack_label_bits")
        for name, key, code, es in (("u8", "labels", _lib.LABEL_U8, 1), ("u16", "u16", _lib.LABEL_U16, 2), ("i32", "i32", _lib.LABEL_I32, 4),
                                    ("rgb8", "rgb8", _lib.LABEL_RGB8, 3)):
            packs[f"b_pack_{name}"] = (P * H * W * es + B * NW * 4, lambda k, key=key, code=code: pack(k, key, code))
            # what the kernel writes is what the timed fits of line (c) read
            pack(0, key, code)
            torch.cuda.synchronize()
            assert torch.equal(bits2, sets[0]["bits"]), name
            assert torch.equal(area.long(), (sets[0]["labels"][sets[0]["ii64"]] == sets[0]["idv"]).flatten(1).sum(1)), name
        lines["d_labels"] = lambda k: la.fit_instances_labels(sets[k % R]["depth"], sets[k % R]["labels"], (sets[k % R]["ids"], sets[k % R]["off"]),
                                                             sets[k % R]["K"])
        blocks_d = [block(s, area_hint=ptr(area)) for s in sets]

        def d_c(k):
            pack(k)
            check(lib.la3d_fit_instances_bits(C.byref(blocks_d[k % R]), ptr(bits2), NW, 0), "bits")
        lines["d_c_pack_then_bits"] = d_c
    return lines, packs, f


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


result = dict(tree=os.path.basename(os.path.abspath(args.root)), have_labels=HAVE_LABELS, build_info=lib.la3d_build_info().decode(),
              device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, us_per_call={}, packers={}, criteria={})
reps = 2 if args.quick else args.reps
for P in ([146] if args.quick else [int(x) for x in args.images.split(",")]):
    B = P * PER
    sets = [make_set(P, 4321 + r) for r in range(R)]
    reader_GBps, _, _ = bench.measured_stream_ceiling([s["labels"] for s in sets])
    lines, packs, fitter = lines_for(P, sets)
    times = {k: [] for k in list(lines) + list(packs)}
    for _ in range(reps):
        for name, fn in lines.items():
            times[name].append(time_line(fn))
        for name, (nbytes, fn) in packs.items():
            times[name].append(time_line(fn))
    torch.cuda.synchronize()
    res = {k: summarise(v) for k, v in times.items() if k in lines}
    result["us_per_call"][str(B)] = res
    pk = {}
    for name, (nbytes, fn) in packs.items():
        s = summarise(times[name])
        s["required_bytes"] = nbytes
        s["GBps_median"] = nbytes / (s["median"] * 1e-6) / 1e9
        pk[name] = s
    result["packers"][str(B)] = dict(pure_reader_GBps=reader_GBps, lines=pk)
    if HAVE_LABELS:
        a, d = res["a_expand_then_u8"], res["d_labels"]
        ac, dc = res["a_c_expand_then_u8"], res["d_c_pack_then_bits"]
        result["criteria"][str(B)] = {
            "d_le_a_by_more_than_a_spread": bool(d["median"] < a["median"] - a["spread"]),
            "a_minus_d_us": a["median"] - d["median"], "a_spread_us": a["spread"], "a_over_d": a["median"] / d["median"],
            "c_entries_d_le_a_by_more_than_a_spread": bool(dc["median"] < ac["median"] - ac["spread"]),
            "c_entries_a_over_d": ac["median"] / dc["median"],
            "mask_bytes_MB": {"a_written_plus_read": 2 * B * H * W / 1e6, "d_labels_read_plus_planes_written_plus_read": (P * H * W + 2 * B * NW * 4) / 1e6},
        }
    del sets, lines, packs, fitter
    torch.cuda.empty_cache()

text = json.dumps(result, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
