"""Measured lines of label maps in the frames call (DESIGN.md section 4.3 "label maps and bit planes of mixed-size images"), every
comparison alternated in ONE process so that the run-to-run spread of each line is known.

    python profiles/frames_bits/measure_frames_bits.py --out profiles/frames_bits/measure_frames_bits.json     # this tree
    python profiles/frames_bits/measure_frames_bits.py --root <checkout of the parent commit> --out ...         # line (a) only

Workload: 256 images over the 18 COCO frame sizes of profiles/frames/measure_frames.py (the same Zipf-like share per size, arrival
order mixed), per image one U8 label map with 7 rectangles of log-uniform area 400 .. 100k px (ids 1 .. 7, later ones painted over
earlier ones) on an unlabeled background, and all 7 ids asked: 1792 instances.  Depth, label maps and K are resident; the ids come
from the host, as a dataset's segments_info does.
(a) the parent commit's only way: the images grouped by frame size, ``fit_instances_labels`` (``la3d_pack_label_bits`` +
    ``la3d_fit_instances_bits``) once per group - 18 pack launches + 18 fit launches and 18 small uploads;
(b) ``fit_instances_frames_labels``: one pack launch, one fit launch, one small upload;
(c) the fit alone: ``fit_instances_frames_bits`` on planes packed beforehand, against ``fit_instances_frames`` on run lengths of the
    same masks (resident), both with the exact areas as ``area_hint``.
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
args = p.parse_args()
sys.path.insert(0, args.root)

import torch  # noqa: E402

import labelany3d_amd as la  # noqa: E402
from labelany3d_amd._lib import lib  # noqa: E402

R, PER_IMAGE = 3, 7
HAVE = hasattr(la, "fit_instances_frames_labels")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()
up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731

COCO_SIZES = [(480, 640), (640, 480), (427, 640), (640, 427), (426, 640), (428, 640), (375, 500), (500, 375), (333, 500), (425, 640),
              (480, 480), (640, 640), (360, 640), (500, 333), (612, 612), (424, 640), (334, 500), (512, 640)]


def rle_of(m):
    flat = m.ravel(order="F")
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return ([0] + counts) if flat[0] else counts


def make_set(seed):
    rs = np.random.RandomState(seed)
    share = 1.0 / np.arange(1, len(COCO_SIZES) + 1)
    share /= share.sum()
    n = np.maximum(1, np.round(share * args.images).astype(int))
    n[0] += args.images - n.sum()
    sizes = [s for s, k in zip(COCO_SIZES, n) for _ in range(k)]
    sizes = [sizes[i] for i in rs.permutation(len(sizes))]                  # arrival order: sizes mixed
    depth, K, labels = [], [], []
    for h, w in sizes:
        vv, uu = np.mgrid[0:h, 0:w]
        depth.append((rs.uniform(2, 6) + rs.uniform(-1e-3, 1e-3) * uu + rs.uniform(0, 3e-3) * vv + 0.02 * rs.randn(h, w)).astype(np.float32))
        f = rs.uniform(450, 650)
        K.append([[f, 0.0, w / 2], [0.0, f, h / 2], [0.0, 0.0, 1.0]])
        lab = np.zeros((h, w), np.uint8)
        for i in range(1, PER_IMAGE + 1):
            area = np.exp(rs.uniform(np.log(400), np.log(100000)))
            asp = np.exp(rs.uniform(-0.6, 0.6))
            hh, ww = int(min(np.sqrt(area * asp), 0.9 * h)), int(min(np.sqrt(area / asp), 0.9 * w))
            r0, c0 = rs.randint(0, h - hh + 1), rs.randint(0, w - ww + 1)
            lab[r0:r0 + hh, c0:c0 + ww] = i
        labels.append(lab)
    return dict(sizes=sizes, depth=depth, K=np.asarray(K), labels=labels, ids=[list(range(1, PER_IMAGE + 1)) for _ in sizes])


def prepare_grouped(s):
    """the parent's way: per frame size the resident (P_g, H, W) depth and label planes, their K and the ids of their images"""
    groups = []
    for size in sorted(set(s["sizes"])):
        imgs = [i for i, z in enumerate(s["sizes"]) if z == size]
        # (the depth rows padded to the next multiple of 32 beforehand, as a caller who keeps depth resident would: no pad launch per call)
        d = np.stack([s["depth"][i] for i in imgs])
        d = np.pad(d, ((0, 0), (0, 0), (0, (-size[1]) % 32)))
        groups.append((up(d), up(np.stack([s["labels"][i] for i in imgs])), [s["ids"][i] for i in imgs], up(s["K"][imgs]), imgs))

    def run():
        out = []
        for d, lab, ids, K, _ in groups:
            out.append(la.fit_instances_labels(d, lab, ids, K))
        return out
    return run, groups


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


result = dict(tree=os.path.relpath(args.root), have_frames_labels=HAVE, build_info=lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0),
              steps=args.steps, warmup=args.warmup, reps=args.reps)
sets = [make_set(311 + r) for r in range(R)]
grouped = [prepare_grouped(s) for s in sets]
lines = {"a_grouped_by_size": lambda k: grouped[k % R][0]()}
if HAVE:
    packed = []
    for s in sets:
        pf, pl, K = la.pack_frames(s["depth"], device=dev), la.pack_label_frames(s["labels"], device=dev), up(s["K"])
        fb = la.pack_label_bits_frames(pl, s["ids"])
        counts, offsets = [], [0]
        for lab, ids in zip(s["labels"], s["ids"]):
            for i in ids:
                counts += rle_of(lab == i)
                offsets.append(len(counts))
        packed.append(dict(pf=pf, pl=pl, K=K, fb=fb, rle=(up(np.asarray(counts, np.int32)), up(np.asarray(offsets, np.int64)))))
    lines["b_one_call"] = lambda k: la.fit_instances_frames_labels(packed[k % R]["pf"], packed[k % R]["pl"], sets[k % R]["ids"], packed[k % R]["K"])
    lines["c_fit_alone_bit_planes"] = lambda k: la.fit_instances_frames_bits(packed[k % R]["pf"], packed[k % R]["fb"], packed[k % R]["K"],
                                                                            area_hint=packed[k % R]["fb"].area)
    lines["c_fit_alone_run_lengths"] = lambda k: la.fit_instances_frames(packed[k % R]["pf"], packed[k % R]["K"], rles=packed[k % R]["rle"],
                                                                         image_index=packed[k % R]["fb"].image_index, area_hint=packed[k % R]["fb"].area)
times = alternate(lines)
torch.cuda.synchronize()
info = dict(images=args.images, frame_sizes=len(set(sets[0]["sizes"])), instances=[sum(len(x) for x in s["ids"]) for s in sets],
            grouped_calls_per_step=[len(g[1]) for g in grouped])
if HAVE:
    # the two ways fit the same instances to the same statuses and records
    for s, g, pk in zip(sets, grouped, packed):
        one = la.fit_instances_frames_labels(pk["pf"], pk["pl"], s["ids"], pk["K"])
        st_one, box_one = one["status"].cpu().numpy().reshape(len(s["sizes"]), PER_IMAGE), one["boxes"].cpu().numpy().reshape(len(s["sizes"]), PER_IMAGE, -1)
        for res, (_, _, _, _, imgs) in zip(g[0](), g[1]):
            assert (res[1].cpu().numpy().reshape(len(imgs), PER_IMAGE) == st_one[imgs]).all(), "the one call and the grouped calls disagree on a status"
            a, b = np.nan_to_num(res[0].cpu().numpy().reshape(len(imgs), PER_IMAGE, -1), nan=-7.0), np.nan_to_num(box_one[imgs], nan=-7.0)
            assert np.allclose(a, b, rtol=1e-9, atol=1e-9), "the one call and the grouped calls disagree on a record"
    info["fitted_fraction"] = float(np.mean([(la.fit_instances_frames_bits(pk["pf"], pk["fb"], pk["K"])["status"] == 0).float().mean().item() for pk in packed]))
    info["b_over_a"] = times["b_one_call"]["median"] / times["a_grouped_by_size"]["median"]
    info["a_minus_b_us"] = times["a_grouped_by_size"]["median"] - times["b_one_call"]["median"]
    info["a_spread_us"] = times["a_grouped_by_size"]["spread"]
result["us_per_step"] = times
result["workload"] = info
text = json.dumps(result, indent=1)
print(text)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
