"""Measured lines of mask overlap on bit planes (include/la3d.h "mask overlap on bit planes"; RESULTS.md beside this file): resident
``MaskBits`` of 640 x 480 -> the per-image overlap matrices and the mask NMS, against what a caller did before - a half-precision
matmul per image on unpacked planes, and a greedy NMS looped on the host with one synchronisation per image -, alternated in ONE
process so that the spread of every line is known (the protocol of profiles/open_bits/bench_open_bits.py).

    python profiles/mask_overlap/bench_mask_overlap.py --out profiles/mask_overlap/bench_mask_overlap.json

Shapes: one image of 16 planes, one of 100, 64 images of 100, 256 images with Poisson(7) planes; each plane the union of three
rectangles or ellipses; ``R`` input sets in rotation (64 x 100 planes are 246 MB of bits per set).
  self            mask_overlap(bits, counts, plan=plan): inter and areas of the self form, tables prepared
  self.iou        the same with iou="iou"
  self.noplan     self without a prepared plan: the tile table is planned on the host and uploaded in the call
  ab.iou          mask_overlap(a, b, ..., iou="iou", plan=plan): A against B (the next set's planes), the full rectangle of tiles
  nms             mask_nms(bits, scores, 0.5, counts): order, self overlap and the NMS kernel, end to end
  nms.given       mask_nms(..., overlap=ov): the order and the NMS kernel alone
  bmm.unpack      unpack_mask_bits -> .half() -> per-image m @ m.T with float32 output (torch.bmm where the counts are equal)
  bmm.u8          the same matmul from u8 planes that are already resident (no unpack): the fairest case for the other side
  nms.torch       greedy NMS without torchvision: the bmm.u8 matrix of an image, copied to the host (one synchronisation per image),
                  and the plain loop there
The shape ``frames<P>x<n>`` is the frames form: P images of the project's mixed-size mix with n planes each, as resident ``FrameBits``
  self / self.iou / ab.iou   as above, through ``mask_overlap(fb, ..., frames=pm, plan=plan)``; no other route is timed for it
Every line is warmed up and timed over ``steps`` calls between two HIP events with the host's clock beside them (``host_us``),
``steps`` raised until a run lasts ``--min-ms``, the lines alternated ``--reps`` times.  Before anything is timed the routes are
compared: inter exactly, keep exactly.  Prints one JSON document."""
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
p.add_argument("--min-ms", type=float, default=50.0, help="a timed run lasts at least this long")
p.add_argument("--shapes", default="1x16,1x100,64x100,256xP7,frames256x7")
args = p.parse_args()
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import labelany3d_amd as la  # noqa: E402

H, W = 480, 640
NW = H * W // 32
VALU_PAIRS_PER_S = 256 * 4 * 32 * 2.4e9 / 2     # word pairs per second at 2 VALU instructions (and, popcount-accumulate) per pair
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
st = torch.cuda.current_stream()


def make_planes(n, seed):
    """(n, H, W) uint8 planes made on the device: unions of three rectangles or ellipses"""
    rs = np.random.RandomState(seed)
    vv = torch.arange(H, device=dev)[:, None]
    uu = torch.arange(W, device=dev)[None, :]
    m = torch.zeros((n, H, W), dtype=torch.bool, device=dev)
    for j in range(n):
        for _ in range(3):
            cy, cx, hy, hx = rs.randint(0, H), rs.randint(0, W), rs.randint(8, H // 3), rs.randint(8, W // 3)
            if rs.rand() < 0.5:
                m[j] |= ((vv - cy).abs() <= hy) & ((uu - cx).abs() <= hx)
            else:
                m[j] |= ((vv - cy) / float(hy)) ** 2 + ((uu - cx) / float(hx)) ** 2 <= 1.0
    return m.view(torch.uint8)


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


def summarise(v):
    runs = sorted(t for t, _ in v)
    return dict(median=float(np.median(runs)), min=runs[0], max=runs[-1], spread=runs[-1] - runs[0], in_order=[t for t, _ in v],
                host_us=float(np.median([h for _, h in v])))


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


try:
    torch.bmm(torch.ones((1, 2, 4), dtype=torch.half, device=dev), torch.ones((1, 4, 2), dtype=torch.half, device=dev), out_dtype=torch.float32)
    F32_OUT = True
except Exception:  # noqa: BLE001 - a torch without the out_dtype form: the half output overflows above 65504 (recorded)
    F32_OUT = False


def gram(m):
    """(n, pixels) or (P, n, pixels) half -> m @ m.T, float32 where torch can (a count of a 640 x 480 frame does not fit a half)"""
    mt = m.transpose(-1, -2)
    if m.dim() == 2:
        return torch.bmm(m[None], mt[None], out_dtype=torch.float32)[0] if F32_OUT else m @ mt
    return torch.bmm(m, mt, out_dtype=torch.float32) if F32_OUT else torch.bmm(m, mt)


def host_nms(inter, scores, thr):
    area = np.diag(inter)
    order = np.argsort(-scores, kind="stable")
    keep, gone = np.zeros(len(scores), bool), np.zeros(len(scores), bool)
    for k, t in enumerate(order):
        if gone[t]:
            continue
        keep[t] = True
        later = order[k + 1:]
        den = area[t] + area[later] - inter[t, later]
        gone[later[(den > 0) & (inter[t, later] > thr * den)]] = True
    return keep


def run_shape(name):
    imgs, per = name.split("x")
    P = int(imgs)
    counts = np.random.RandomState(11).poisson(7, P).astype(np.int64) if per.startswith("P") else np.full(P, int(per), np.int64)
    B = int(counts.sum())
    equal = not per.startswith("P")
    R = 2 if B * NW * 4 > 64e6 else 4
    rows = np.concatenate([[0], np.cumsum(counts)])
    u8 = [make_planes(B, 1000 + 17 * r) for r in range(R)]
    bits = [la.pack_mask_bits(m) for m in u8]
    scores = [torch.rand(B, device=dev, generator=torch.Generator(device=dev).manual_seed(r)) for r in range(R)]
    clist = counts.tolist()
    plan_s = la.mask_overlap_plan(bits[0], None, clist)
    plan_ab = la.mask_overlap_plan(bits[0], bits[1], clist, clist)

    def bmm_of(planes):
        h = planes.half().flatten(1)
        if equal:
            return gram(h.view(P, int(counts[0]), -1))
        return [gram(h[rows[g]:rows[g + 1]]) for g in range(P) if counts[g]]

    def nms_torch(k):
        out = []
        h = u8[k % R]
        s = scores[k % R]
        for g in range(P):
            if counts[g]:
                inter = gram(h[rows[g]:rows[g + 1]].half().flatten(1)).cpu().numpy()       # one synchronisation per image
                out.append(host_nms(inter, s[rows[g]:rows[g + 1]].cpu().numpy(), 0.5))
        return out

    # the routes agree before anything is timed
    ov = la.mask_overlap(bits[0], counts_a=clist, plan=plan_s)
    got = ov.inter.cpu().numpy()
    want = bmm_of(u8[0])
    want = np.concatenate([w.reshape(-1).cpu().numpy() for w in (want if isinstance(want, list) else [want])])
    exact = bool(F32_OUT and (got == want).all())
    keep = la.mask_nms(bits[0], scores[0], 0.5, counts=clist).cpu().numpy()
    ref_keep = np.concatenate(nms_torch(0)) if B else np.zeros(0, bool)
    keep_equal = bool((keep == ref_keep).all()) if F32_OUT else None
    ovs = [la.mask_overlap(b, counts_a=clist, plan=plan_s) for b in bits]
    torch.cuda.synchronize()

    lines = {
        "self": lambda k: la.mask_overlap(bits[k % R], counts_a=clist, plan=plan_s),
        "self.iou": lambda k: la.mask_overlap(bits[k % R], counts_a=clist, iou="iou", plan=plan_s),
        "self.noplan": lambda k: la.mask_overlap(bits[k % R], counts_a=clist),
        "ab.iou": lambda k: la.mask_overlap(bits[k % R], bits[(k + 1) % R], clist, clist, iou="iou", plan=plan_ab),
        "nms": lambda k: la.mask_nms(bits[k % R], scores[k % R], 0.5, counts=clist),
        "nms.given": lambda k: la.mask_nms(bits[k % R], scores[k % R], 0.5, counts=clist, overlap=ovs[k % R]),
        "bmm.unpack": lambda k: bmm_of(la.unpack_mask_bits(bits[k % R])),
        "bmm.u8": lambda k: bmm_of(u8[k % R]),
        "nms.torch": nms_torch,
    }
    steps = {}
    for key, fn in lines.items():
        t, _ = time_device(fn, 2, 2)
        steps[key] = int(min(max(2, np.ceil(args.min_ms * 1e3 / max(t, 1.0))), 2000))
    raw = {key: [] for key in lines}
    for _ in range(args.reps):
        for key, fn in lines.items():
            raw[key].append(time_device(fn, steps[key], 2))
    res = {key: dict(summarise(v), steps=steps[key]) for key, v in raw.items()}
    useful = float((counts * counts).sum()) * NW                       # word pairs of the full matrices
    done_self = float((plan_s.tiles_host["chunk"] == 0).sum()) * 64 * NW   # computed: 8 x 8 pairs per tile, edge tiles included
    done_ab = float((plan_ab.tiles_host["chunk"] == 0).sum()) * 64 * NW
    rates = dict(useful_pairs_per_s_self=useful / (res["self"]["median"] * 1e-6), computed_pairs_per_s_self=done_self / (res["self"]["median"] * 1e-6),
                 computed_pairs_per_s_ab=done_ab / (res["ab.iou"]["median"] * 1e-6), valu_peak_pairs_per_s=VALU_PAIRS_PER_S)
    rates["share_of_valu_peak_self"] = rates["computed_pairs_per_s_self"] / VALU_PAIRS_PER_S
    rates["share_of_valu_peak_ab"] = rates["computed_pairs_per_s_ab"] / VALU_PAIRS_PER_S
    del u8, bits, ovs
    torch.cuda.empty_cache()
    return dict(images=P, planes=B, sets=R, bits_mb_per_set=B * NW * 4 / 1e6, tiles_self=len(plan_s.tiles_host), tiles_ab=len(plan_ab.tiles_host),
                chunks_self=int(plan_s.tiles_host["nchunks"].max()) if len(plan_s.tiles_host) else 0, inter_equals_bmm=exact,
                keep_equals_host_loop=keep_equal, kept=int(keep.sum()), lines_us=res, rates=rates)


def run_frames(name):
    """the frames form on the mixed-size mix; before anything is timed three images are compared with the uniform call on them alone"""
    imgs, per = name[len("frames"):].split("x")
    P, per = int(imgs), int(per)
    sizes = coco_mix(P, 7)
    R = 2
    stacks = [make_stacks(sizes, per, 3100 + r) for r in range(R)]
    pms = [la.pack_mask_frames(x) for x in stacks]
    fbs = [la.pack_mask_bits_frames(pm) for pm in pms]
    clist = [per] * P
    plan_s = la.mask_overlap_plan(fbs[0], None, clist, frames=pms[0])
    plan_ab = la.mask_overlap_plan(fbs[0], fbs[1], clist, clist, frames=pms[0])
    ov = la.mask_overlap(fbs[0], counts_a=clist, frames=pms[0], plan=plan_s)
    exact = all(bool((ov.matrix(g) == la.mask_overlap(la.pack_mask_bits(stacks[0][g])).matrix(0)).all()) for g in (0, P // 2, P - 1))
    assert exact and int((ov.area_a < 0).sum()) == 0
    lines = {
        "self": lambda k: la.mask_overlap(fbs[k % R], counts_a=clist, frames=pms[k % R], plan=plan_s),
        "self.iou": lambda k: la.mask_overlap(fbs[k % R], counts_a=clist, frames=pms[k % R], iou="iou", plan=plan_s),
        "ab.iou": lambda k: la.mask_overlap(fbs[k % R], fbs[(k + 1) % R], clist, clist, frames=pms[k % R], iou="iou", plan=plan_ab),
    }
    steps = {}
    for key, fn in lines.items():
        t, _ = time_device(fn, 2, 2)
        steps[key] = int(min(max(2, np.ceil(args.min_ms * 1e3 / max(t, 1.0))), 2000))
    raw = {key: [] for key in lines}
    for _ in range(args.reps):
        for key, fn in lines.items():
            raw[key].append(time_device(fn, steps[key], 2))
    res = {key: dict(summarise(v), steps=steps[key]) for key, v in raw.items()}
    return dict(images=P, planes=P * per, sets=R, distinct_sizes=len(set(sizes)), tiles_self=len(plan_s.tiles_host), tiles_ab=len(plan_ab.tiles_host),
                inter_equals_uniform=exact, lines_us=res)


doc = dict(build_info=la._lib.lib.la3d_build_info().decode(), device=torch.cuda.get_device_name(0), torch=torch.__version__, frame=[H, W], words=NW, bmm_float32_output=F32_OUT,
           reps=args.reps, min_ms=args.min_ms, shapes={})
for shape in args.shapes.split(","):
    doc["shapes"][shape] = run_frames(shape) if shape.startswith("frames") else run_shape(shape)
    print(shape, json.dumps({k: round(v["median"], 1) for k, v in doc["shapes"][shape]["lines_us"].items()}), flush=True)
text = json.dumps(doc, indent=1)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
print(json.dumps(doc))
