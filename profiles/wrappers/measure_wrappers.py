"""Host time of the Python wrappers of the depth + mask fit: wall clock per call, each call ending in a device synchronise, warmed
up.  Nothing here can see a kernel get slower or faster - the library is the same -; what it sees is Python work on the per-image
path, where the fit is ~40 us inside 100 - 200 us of wrapper.

    python profiles/wrappers/measure_wrappers.py --out run.json                       # the lines of this tree
    python profiles/wrappers/measure_wrappers.py --root <other checkout> --out ...    # ... of another one (its labelany3d_amd)
    python profiles/wrappers/measure_wrappers.py --compare <parent checkout> --out profiles/wrappers/measure_wrappers.json

``--compare`` runs parent, this tree, parent, this tree (``--alternations`` pairs, default 2), each in a fresh child process, and judges
every line: this tree's median over its runs may not exceed the parent's median by more than the spread (max - min) between the
parent's own runs.  It prints the table of RESULTS.md.

Lines (us per call, the median of ``--reps`` calls after ``--warmup``):
  annotations_host_<WxH> / annotations_device_<WxH>   ``fit_annotations(to_host=True / False)`` on an image of 8 annotations (6 polygons,
                              2 run-length masks, all with ``area``), depth resident: 640x480, and 427x640 (odd width: padded per call)
  ex_rle_B8 / ex_rle_B1024    ``fit_instances_ex(rles=pack_rle tuple)`` on one shared 640x480 plane
  bits_B1022 / labels_B1022   ``fit_instances_bits`` on resident planes / ``fit_instances_labels`` on 146 resident U8 label maps x 7 ids
  frames_poly / frames_rle    ``fit_instances_frames`` on 256 images of 18 COCO sizes (the set of profiles/frames), ~7 instances each
  open_bits_frames_B8 / components_bits_frames_B8 / rle_encode_bits_frames_B8 / mask_overlap_frames_B8
                              the plane operations on the ``FrameBits`` of 8 masks over 3 images of different sizes (7 x 7 opening,
                              largest component, encoder with ``capacity=int``, self IoU): the batch where host time is the call
  run_B1024                   the bare ``InstanceFitter.run`` enqueue, everything resident"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
p = argparse.ArgumentParser()
p.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)))
p.add_argument("--compare", default=None, metavar="PARENT_ROOT")
p.add_argument("--out", default=None)
p.add_argument("--reps", type=int, default=200)
p.add_argument("--warmup", type=int, default=20)
p.add_argument("--images", type=int, default=256)
p.add_argument("--alternations", type=int, default=2)
args = p.parse_args()

# (H, W) of COCO images by falling frequency (profiles/frames/measure_frames.py)
COCO_SIZES = [(480, 640), (640, 480), (427, 640), (640, 427), (426, 640), (428, 640), (375, 500), (500, 375), (333, 500), (425, 640),
              (480, 480), (640, 640), (360, 640), (500, 333), (612, 612), (424, 640), (334, 500), (512, 640)]
K640 = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])


def rle_of(m):
    flat = m.ravel(order="F")
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return ([0] + counts) if flat[0] else counts


def ellipse(rs, h, w):
    """(centre, half axes) of an ellipse of log-uniform area inside an h x w frame, clear of the boundary strip"""
    area = np.exp(rs.uniform(np.log(400), np.log(60000)))
    asp = np.exp(rs.uniform(-0.6, 0.6))
    hh, ww = min(np.sqrt(area * asp), 0.8 * h), min(np.sqrt(area / asp), 0.8 * w)
    return rs.uniform(hh / 2 + 12, h - hh / 2 - 12), rs.uniform(ww / 2 + 12, w - ww / 2 - 12), hh / 2, ww / 2


def ellipse_mask(e, h, w):
    vv, uu = np.mgrid[0:h, 0:w]
    return ((vv - e[0]) / e[2]) ** 2 + ((uu - e[1]) / e[3]) ** 2 <= 1.0


def ellipse_polygon(e):
    ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
    return np.stack([e[1] + e[3] * np.cos(ang), e[0] + e[2] * np.sin(ang)], 1)


def measure():
    sys.path.insert(0, args.root)
    import torch

    import labelany3d_amd as la

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rs = np.random.RandomState(7)
    lines = {}

    def plane(n, h, w):
        g = torch.Generator(device=dev)
        g.manual_seed(n * 1000 + w)
        return torch.empty((n, h, w), dtype=torch.float32, device=dev).uniform_(1.0, 8.0, generator=g)

    # ---- the per-image path
    for W, H in ((640, 480), (427, 640)):
        ann = []
        for n in range(8):
            e = ellipse(rs, H, W)
            m = ellipse_mask(e, H, W)
            seg = {"size": [H, W], "counts": rle_of(m)} if n % 4 == 3 else [ellipse_polygon(e).ravel().tolist()]
            ann.append({"segmentation": seg, "area": float(m.sum()), "bbox": [0, 0, 1, 1], "category_id": n, "iscrowd": 0})
        d = plane(1, H, W)[0]
        lines[f"annotations_host_{W}x{H}"] = lambda ann=ann, W=W, H=H, d=d: la.fit_annotations(ann, (W, H), d, K640, to_host=True)
        lines[f"annotations_device_{W}x{H}"] = lambda ann=ann, W=W, H=H, d=d: la.fit_annotations(ann, (W, H), d, K640)

    # ---- fit_instances_ex with run lengths, one shared plane
    H, W = 480, 640
    d1 = plane(1, H, W)
    masks = np.stack([ellipse_mask(ellipse(rs, H, W), H, W) for _ in range(64)])
    for B in (8, 1024):
        packed = la.pack_rle([{"size": [H, W], "counts": rle_of(masks[n % 64])} for n in range(B)])
        lines[f"ex_rle_B{B}"] = lambda packed=packed: la.fit_instances_ex(d1, K640, rles=packed)

    # ---- bit planes and label maps: 146 images x 7 ids
    P, PER = 146, 7
    labels = np.zeros((P, H, W), np.uint8)
    for pi in range(P):
        for k in range(1, PER + 1):
            h, w = rs.randint(20, 200), rs.randint(20, 300)
            r0, c0 = rs.randint(0, H - h), rs.randint(0, W - w)
            labels[pi, r0:r0 + h, c0:c0 + w] = k
    dP, lab_t = plane(P, H, W), torch.as_tensor(labels, device=dev)
    ids = [list(range(1, PER + 1))] * P
    lb = la.pack_label_bits(lab_t, ids)
    KP = np.stack([K640] * P)
    lines["bits_B1022"] = lambda: la.fit_instances_bits(dP, lb.bits, KP, image_index=lb.image_index, area_hint=lb.area)
    lines["labels_B1022"] = lambda: la.fit_instances_labels(dP, lab_t, ids, KP)

    # ---- images of different sizes in one call
    share = 1.0 / np.arange(1, len(COCO_SIZES) + 1)
    n = np.maximum(1, np.round(share / share.sum() * args.images).astype(int))
    n[0] += args.images - n.sum()
    sizes = [s for s, k in zip(COCO_SIZES, n) for _ in range(k)]
    sizes = [sizes[i] for i in rs.permutation(len(sizes))]
    maps, Ks, segs, rles, img_p, img_r, area_p, area_r = [], [], [], [], [], [], [], []
    for pi, (h, w) in enumerate(sizes):
        maps.append(rs.uniform(1.0, 8.0, (h, w)).astype(np.float32))
        Ks.append([[500.0, 0, w / 2], [0, 500.0, h / 2], [0, 0, 1]])
        for j in range(max(1, rs.poisson(7.0))):
            e = ellipse(rs, h, w)
            if pi % 8 == 0 and j == 0:
                m = ellipse_mask(e, h, w)
                rles.append({"size": [h, w], "counts": rle_of(m)}); img_r.append(pi); area_r.append(int(m.sum()))
            else:
                segs.append([ellipse_polygon(e).ravel().tolist()]); img_p.append(pi); area_p.append(int(np.pi * e[2] * e[3]))
    pf = la.pack_frames(maps, device=dev)
    Ks = np.asarray(Ks)
    polys = la.pack_polygons(segs, max(h for h, _ in sizes), max(w for _, w in sizes))
    counts, offsets, _ = la.masks.pack_rle_frames(rles)
    img_p, img_r, area_p, area_r = (np.asarray(v, np.int32) for v in (img_p, img_r, area_p, area_r))
    lines["frames_poly"] = lambda: la.fit_instances_frames(pf, Ks, polys=polys, image_index=img_p, area_hint=area_p, filter=True, proj=True)
    lines["frames_rle"] = lambda: la.fit_instances_frames(pf, Ks, rles=(counts, offsets), image_index=img_r, area_hint=area_r)

    # ---- plane operations on FrameBits at the small batch where host time is the call: 8 planes over 3 images of different sizes
    small_sizes, per_image = [(480, 640), (375, 500), (333, 500)], [3, 3, 2]
    pm = la.pack_mask_frames([np.stack([ellipse_mask(ellipse(rs, h, w), h, w) for _ in range(c)]) for (h, w), c in zip(small_sizes, per_image)],
                             device=dev)
    fb = la.pack_mask_bits_frames(pm)
    lines["open_bits_frames_B8"] = lambda: la.open_bits_frames(pm, fb, k=7)
    lines["components_bits_frames_B8"] = lambda: la.components_bits_frames(pm, fb, largest=True)
    lines["rle_encode_bits_frames_B8"] = lambda: la.rle_encode_bits_frames(pm, fb, capacity=65536)
    lines["mask_overlap_frames_B8"] = lambda: la.mask_overlap(fb, counts_a=per_image, frames=pm, iou="iou")

    # ---- the bare enqueue
    B = 1024
    f = la.InstanceFitter(B, H, W)
    mt = torch.as_tensor(masks, device=dev).view(torch.uint8)[torch.arange(B, device=dev) % 64].contiguous()
    kt = torch.as_tensor(K640, device=dev)
    lines["run_B1024"] = lambda: f.run(d1[0], mt, kt)

    out = {}
    for name, fn in lines.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e6)
        out[name] = dict(median=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)))
    return dict(root=os.path.basename(os.path.abspath(args.root)), device=torch.cuda.get_device_name(0), arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                build_info=la._lib.lib.la3d_build_info().decode(), reps=args.reps, warmup=args.warmup, us_per_call=out)


def compare():
    runs = []
    for who, root in (("parent", args.compare), ("branch", args.root)) * args.alternations:
        tmp = f"{args.out or os.path.join(HERE, 'measure_wrappers.json')}.{len(runs)}.tmp"
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--out", tmp, "--reps", str(args.reps),
                             "--warmup", str(args.warmup), "--images", str(args.images)], stdout=subprocess.DEVNULL, timeout=600).returncode
        if rc != 0:
            raise SystemExit(f"the {who} run ended with status {rc}: nothing more is started")
        with open(tmp) as fh:
            runs.append(dict(json.load(fh), who=who))
        os.remove(tmp)
    verdict, rows = {}, []
    for name in runs[0]["us_per_call"]:
        pa, br = ([r["us_per_call"][name]["median"] for r in runs if r["who"] == w] for w in ("parent", "branch"))
        spread = max(pa) - min(pa)
        bound = float(np.median(pa) + spread)
        verdict[name] = dict(parent=pa, branch=br, parent_median=float(np.median(pa)), parent_spread=spread,
                             branch_median=float(np.median(br)), bound=bound, within=bool(np.median(br) <= bound))
        rows.append(f"| `{name}` | {' '.join(f'{v:.1f}' for v in pa)} | {' '.join(f'{v:.1f}' for v in br)} | {np.median(pa):.1f} + {spread:.1f} | "
                    f"{np.median(br):.1f} | {'within' if verdict[name]['within'] else '**SLOWER**'} |")
    print("| line | parent runs | branch runs | bound (parent median + spread) | branch median | verdict |")
    print("|---|---|---|---|---|---|")
    print("\n".join(rows))
    return dict(order=[r["who"] for r in runs], runs=runs, verdict=verdict, all_within=all(v["within"] for v in verdict.values()))


result = compare() if args.compare else measure()
text = json.dumps(result, indent=1)
if not args.compare:
    print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
