"""Measured lines of network masks and logits in the frames call (DESIGN.md section 4.3 "network masks and logits of mixed-size
images"), every comparison alternated in ONE process so that the run-to-run spread of each line is known.

    python profiles/frames_masks/measure_frames_masks.py --out profiles/frames_masks/measure_frames_masks.json

Workload: that of profiles/frames_bits/measure_frames_bits.py - 256 images over the 18 COCO frame sizes (the same Zipf-like share
per size, arrival order mixed), per image 7 rectangles of log-uniform area 400 .. 100k px: 1792 instances -, here as what an
instance-segmentation network hands over: per image ONE resident (7, H_p, W_p) tensor, uint8 masks or float16 logits (+-1).  Depth,
masks and K are resident.
(a) ``pack_mask_bits_frames`` (one launch over the planes where they lie) + one ``fit_instances_frames_bits`` call;
(b) what the parent commit can do: the images grouped by frame size, ``pack_mask_bits`` / ``pack_logits_bits`` + ``fit_instances_bits``
    once per group - 18 pack launches + 18 fit launches;
(c) per frame size ``fit_instances`` on the u8 planes (no packing at all; u8 only).
The packer alone: ``pack_mask_bits_frames`` on the images whose width is a multiple of 16 (every plane in 16-byte groups) and on the
images of odd width (427, 375, 333, 425: every plane element by element), each next to ``pack_mask_bits`` / ``pack_logits_bits`` on
the same number of bytes in ONE uniform (480, 640) size; GB/s = source bytes read per second.
Three resident input sets in rotation (seeds + 0 / 1 / 2), 5 warm-up + 20 timed steps per line between two HIP events, the lines
alternated ``--reps`` times (default 6); median, min, max and spread (max - min) of every line are reported."""
import argparse
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
p.add_argument("--sets", type=int, default=3)
args = p.parse_args()
sys.path.insert(0, args.root)

import torch  # noqa: E402

import labelany3d_amd as la  # noqa: E402
from labelany3d_amd._lib import lib  # noqa: E402

R, PER_IMAGE = args.sets, 7
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()
up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731

COCO_SIZES = [(480, 640), (640, 480), (427, 640), (640, 427), (426, 640), (428, 640), (375, 500), (500, 375), (333, 500), (425, 640),
              (480, 480), (640, 640), (360, 640), (500, 333), (612, 612), (424, 640), (334, 500), (512, 640)]


def make_set(seed):
    rs = np.random.RandomState(seed)
    share = 1.0 / np.arange(1, len(COCO_SIZES) + 1)
    share /= share.sum()
    n = np.maximum(1, np.round(share * args.images).astype(int))
    n[0] += args.images - n.sum()
    sizes = [s for s, k in zip(COCO_SIZES, n) for _ in range(k)]
    sizes = [sizes[i] for i in rs.permutation(len(sizes))]                  # arrival order: sizes mixed
    depth, K, masks = [], [], []
    for h, w in sizes:
        vv, uu = np.mgrid[0:h, 0:w]
        depth.append((rs.uniform(2, 6) + rs.uniform(-1e-3, 1e-3) * uu + rs.uniform(0, 3e-3) * vv + 0.02 * rs.randn(h, w)).astype(np.float32))
        f = rs.uniform(450, 650)
        K.append([[f, 0.0, w / 2], [0.0, f, h / 2], [0.0, 0.0, 1.0]])
        m = np.zeros((PER_IMAGE, h, w), np.uint8)
        for i in range(PER_IMAGE):
            area = np.exp(rs.uniform(np.log(400), np.log(100000)))
            asp = np.exp(rs.uniform(-0.6, 0.6))
            hh, ww = int(min(np.sqrt(area * asp), 0.9 * h)), int(min(np.sqrt(area / asp), 0.9 * w))
            r0, c0 = rs.randint(0, h - hh + 1), rs.randint(0, w - ww + 1)
            m[i, r0:r0 + hh, c0:c0 + ww] = 1
        masks.append(m)
    return dict(sizes=sizes, depth=depth, K=np.asarray(K), masks=masks)


def resident(s):
    """per image one device tensor, as a network leaves them: uint8 masks and float16 logits"""
    u8 = [up(m) for m in s["masks"]]
    f16 = [(t.to(torch.float16) * 2 - 1) for t in u8]
    return u8, f16


def prepare_grouped(s, u8, f16):
    """the parent's way: per frame size the resident (P_g, H, padded W) depth, the (7 P_g, H, W) planes of its images and their K"""
    groups = []
    for size in sorted(set(s["sizes"])):
        imgs = [i for i, z in enumerate(s["sizes"]) if z == size]
        d = np.stack([s["depth"][i] for i in imgs])
        ii = up(np.repeat(np.arange(len(imgs)), PER_IMAGE).astype(np.int32))
        groups.append(dict(depth=up(d), depth_padded=up(np.pad(d, ((0, 0), (0, 0), (0, (-size[1]) % 32)))), u8=torch.cat([u8[i] for i in imgs]),
                           f16=torch.cat([f16[i] for i in imgs]), K=up(s["K"][imgs]), ii=ii, imgs=imgs))

    def run_bits(kind):
        out = []
        for g in groups:
            mb = la.pack_mask_bits(g["u8"]) if kind == "u8" else la.pack_logits_bits(g["f16"])
            out.append(la.fit_instances_bits(g["depth_padded"], mb, g["K"], image_index=g["ii"]))
        return out

    def run_u8():
        return [la.fit_instances(g["depth"], g["u8"], g["K"], image_index=g["ii"]) for g in groups]

    return dict(groups=groups, run_bits=run_bits, run_u8=run_u8)


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


def one_call(pk, kind):
    fb = la.pack_mask_bits_frames(pk[kind], out=pk["out"])
    return la.fit_instances_frames_bits(pk["pf"], fb, pk["K"], area_hint=fb.area)


result = dict(build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, reps=args.reps)
sets = [make_set(311 + r) for r in range(R)]
packed, grouped = [], []
for s in sets:
    u8, f16 = resident(s)
    pm8, pm16 = la.pack_mask_frames(u8), la.pack_mask_frames(f16)
    assert pm8.sources and pm16.sources, "the resident stacks must be read where they lie"
    packed.append(dict(pf=la.pack_frames(s["depth"], device=dev), K=up(s["K"]), u8=pm8, f16=pm16,
                       out=torch.empty(pm8.bits_words, dtype=torch.int32, device=dev), stacks=(u8, f16)))
    grouped.append(prepare_grouped(s, u8, f16))
lines = {}
for kind in ("u8", "f16"):
    lines[f"a_one_call_{kind}"] = lambda k, kind=kind: one_call(packed[k % R], kind)
    lines[f"b_grouped_by_size_{kind}"] = lambda k, kind=kind: grouped[k % R]["run_bits"](kind)
lines["c_grouped_fit_instances_u8"] = lambda k: grouped[k % R]["run_u8"]()

# the packer alone: the aligned and the odd-width images of every set, and the uniform packers on the same number of bytes
alone = {}
for name, want in (("aligned", lambda w: w % 16 == 0), ("odd_width", lambda w: w % 2 == 1)):
    for kind, idx in (("u8", 0), ("f16", 1)):
        pms = []
        for s, pk in zip(sets, packed):
            pms.append(la.pack_mask_frames([t for t, (h, w) in zip(pk["stacks"][idx], s["sizes"]) if want(w)]))
        nbytes = [sum(c * h * w for c, (h, w) in zip([PER_IMAGE] * len(pm.sizes), pm.sizes)) * pm.data.element_size() for pm in pms]
        outs = [torch.empty(pm.bits_words, dtype=torch.int32, device=dev) for pm in pms]
        planes = int(round(np.mean(nbytes) / pms[0].data.element_size() / (480 * 640)))
        uni = torch.ones((planes, 480, 640), dtype=pms[0].data.dtype, device=dev)
        uni_out = torch.empty((planes, 480 * 640 // 32), dtype=torch.int32, device=dev)
        alone[f"pack_frames_{name}_{kind}"] = dict(bytes=float(np.mean(nbytes)), planes=int(np.mean([pm.offsets.numel() for pm in pms])))
        alone[f"pack_uniform_{name}_{kind}"] = dict(bytes=float(uni.numel() * uni.element_size()), planes=planes)
        lines[f"pack_frames_{name}_{kind}"] = lambda k, pms=pms, outs=outs: la.pack_mask_bits_frames(pms[k % R], out=outs[k % R])
        lines[f"pack_uniform_{name}_{kind}"] = (lambda k, uni=uni, uni_out=uni_out: la.pack_mask_bits(uni, out=uni_out)) if kind == "u8" else \
            (lambda k, uni=uni, uni_out=uni_out: la.pack_logits_bits(uni, out=uni_out))
for kind in ("u8", "f16"):
    lines[f"pack_frames_workload_{kind}"] = lambda k, kind=kind: la.pack_mask_bits_frames(packed[k % R][kind], out=packed[k % R]["out"])
    alone[f"pack_frames_workload_{kind}"] = dict(bytes=float(np.mean([sum(PER_IMAGE * h * w for h, w in s["sizes"]) for s in sets]) * (1 if kind == "u8" else 2)),
                                                 planes=PER_IMAGE * args.images)
times = alternate(lines)
torch.cuda.synchronize()
for name, a in alone.items():
    a["us"] = times[name]["median"]
    a["GB_per_s"] = a["bytes"] / (a["us"] * 1e-6) / 1e9

# the ways fit the same instances to the same statuses and records
info = dict(images=args.images, frame_sizes=len(set(sets[0]["sizes"])), instances=[PER_IMAGE * len(s["sizes"]) for s in sets],
            grouped_calls_per_step=[len(g["groups"]) for g in grouped])
for s, g, pk in zip(sets, grouped, packed):
    for kind in ("u8", "f16"):
        one = one_call(pk, kind)
        st_one = one["status"].cpu().numpy().reshape(len(s["sizes"]), PER_IMAGE)
        box_one = one["boxes"].cpu().numpy().reshape(len(s["sizes"]), PER_IMAGE, -1)
        for res, grp in zip(g["run_bits"](kind), g["groups"]):
            imgs = grp["imgs"]
            assert (res[1].cpu().numpy().reshape(len(imgs), PER_IMAGE) == st_one[imgs]).all(), "the one call and the grouped calls disagree on a status"
            a, b = np.nan_to_num(res[0].cpu().numpy().reshape(len(imgs), PER_IMAGE, -1), nan=-7.0), np.nan_to_num(box_one[imgs], nan=-7.0)
            assert np.allclose(a, b, rtol=1e-9, atol=1e-9), "the one call and the grouped calls disagree on a record"
info["fitted_fraction"] = float(np.mean([(one_call(pk, "u8")["status"] == 0).float().mean().item() for pk in packed]))
for kind in ("u8", "f16"):
    info[f"a_over_b_{kind}"] = times[f"a_one_call_{kind}"]["median"] / times[f"b_grouped_by_size_{kind}"]["median"]
info["a_over_c_u8"] = times["a_one_call_u8"]["median"] / times["c_grouped_fit_instances_u8"]["median"]
result["us_per_step"] = times
result["packer_alone"] = alone
result["workload"] = info
text = json.dumps(result, indent=1)
print(text)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
