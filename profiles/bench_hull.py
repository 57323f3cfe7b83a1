"""Timing of the convex-hull yaw on the fused depth + mask path: per 1024 instances of 640 x 480,
u8 planes and run lengths, full-mask and reference-subsample mode -

  * the hull call next to the PCA call of the same inputs (both launches of the hull call);
  * the hull call next to the only route there was before it: unproject every plane, gather every mask in torch,
    ``fit_points(method="convex_hull")`` with 500 drawn ranks per instance.

Protocol: R resident input batches, timed step k reads batch k % R (no two consecutive steps read the same bytes); W warm-up
steps; K timed steps between two device synchronisations, repeated `--repeats` times with the variants ALTERNATING; the median
and the range of the repeats are reported.  One JSON line.  The finish kernel alone: run this script with ``--only hull`` under
``rocprofv3 --kernel-trace --stats -- python profiles/bench_hull.py ...`` (a run of its own).

    python profiles/bench_hull.py --B 1024 --steps 20 --warmup 5 --repeats 3
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_batch(seed, B, H, W, dev):
    """elliptic masks on private noisy sloped depth planes (the shape of BASELINE config 2), generated on the device"""
    import torch

    g = torch.Generator(device=dev).manual_seed(seed)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g, device=dev) * (hi - lo) + lo   # noqa: E731
    vv = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
    uu = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
    depth = (u(2, 5, B, 1, 1) + u(-0.004, 0.004, B, 1, 1) * uu + u(-0.003, 0.003, B, 1, 1) * vv
             + 0.05 * torch.randn(B, H, W, generator=g, device=dev)).contiguous()
    cy, cx = u(0.25, 0.75, B, 1, 1) * H, u(0.25, 0.75, B, 1, 1) * W
    ry, rx = u(0.08, 0.24, B, 1, 1) * H, u(0.08, 0.24, B, 1, 1) * W
    masks = (((vv - cy) / ry) ** 2 + ((uu - cx) / rx) ** 2 <= 1.0).to(torch.uint8).contiguous()
    return depth, masks


def rle_of(masks):
    """uncompressed COCO run lengths (column-major, zeros first) of u8 planes, packed as pack_rle does"""
    m = masks.cpu().numpy().astype(bool)
    counts, offsets = [], [0]
    for x in m:
        flat = x.ravel(order="F")
        change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
        c = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
        counts += ([0] + c) if flat[0] else c
        offsets.append(len(counts))
    return np.asarray(counts, np.int32), np.asarray(offsets, np.int64)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--H", type=int, default=480)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--only", default=None, help="time one variant only (e.g. hull_u8_full), for a profiler run")
    ap.add_argument("--skip-old-route", action="store_true")
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_hull.py measures on the GPU: no device visible")
    import labelany3d_amd as la
    from labelany3d_amd import InstanceFitter
    from labelany3d_amd.batched import _fit_args, _ptr, _stream
    from labelany3d_amd._lib import METHOD_CONVEX_HULL, METHOD_PCA, check, lib
    import ctypes as C

    dev = torch.device("cuda", 0)
    B, H, W, R = args.B, args.H, args.W, args.rotate
    K = torch.tensor([[500.0, 0, W / 2.0], [0, 500.0, H / 2.0], [0, 0, 1]], dtype=torch.float64, device=dev)
    batches = []
    for r in range(R):
        depth, masks = make_batch(1000 + r, B, H, W, dev)
        c, o = rle_of(masks)
        counts = masks.reshape(B, -1).sum(1).cpu().numpy()
        sidx = torch.as_tensor(la.draw_sample_idx(counts, np.random.RandomState(r)), device=dev)
        batches.append(dict(depth=depth, masks=masks, rle=(torch.as_tensor(c, device=dev), torch.as_tensor(o, device=dev)), sidx=sidx,
                            counts=torch.as_tensor(counts, device=dev)))
    f = InstanceFitter(B, H, W, dev, method="convex_hull")

    def fit(b, method, rle, sample):
        kind = dict(rle=(_ptr(b["rle"][0]), _ptr(b["rle"][1]))) if rle else dict(mask=_ptr(b["masks"]))
        a = _fit_args(B, H, W, _ptr(b["depth"]), B, _ptr(K), 1, _ptr(f.boxes[0]), _ptr(f.status[0]), _ptr(f.aux[0]), _ptr(f.workspace[0]),
                      _stream(None), sample_idx=_ptr(b["sidx"]) if sample else None, method=method, **kind)
        check(lib.la3d_fit_instances_ex(C.byref(a)), "la3d_fit_instances_ex")

    def old_route(b):
        """what a user had to do before: unproject, gather every mask, fit_points(convex_hull) on 500 drawn ranks per instance"""
        pts = la.unproject(b["depth"], K)                                  # (B,H,W,3) f64
        sel = b["masks"].view(torch.bool)
        cloud = pts[sel]                                                   # row-major order of the True pixels, instance after instance
        off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(b["counts"], 0)
        la.fit_points((cloud, off), sample_idx=b["sidx"], method="convex_hull")

    variants = {}
    for src in ("u8", "rle"):
        for mode in ("full", "sample"):
            for name, meth in (("pca", METHOD_PCA), ("hull", METHOD_CONVEX_HULL)):
                variants[f"{name}_{src}_{mode}"] = (lambda b, m=meth, s=src, md=mode: fit(b, m, s == "rle", md == "sample"))
    if not args.skip_old_route:
        variants["old_route_u8_sample"] = old_route
    if args.only:
        variants = {args.only: variants[args.only]}

    def timed(fn):
        for k in range(args.warmup):
            fn(batches[k % R])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.steps):
            fn(batches[k % R])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e6

    us = {k: [] for k in variants}
    for _ in range(args.repeats):        # the variants alternate inside every repeat
        for k, fn in variants.items():
            us[k].append(timed(fn))
    out = {"B": B, "H": H, "W": W, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "rotate": R,
           "us_per_call": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in us.items()}}
    m = lambda k: out["us_per_call"][k]["median"]   # noqa: E731
    if not args.only:
        out["hull_over_pca"] = {f"{s}_{md}": m(f"hull_{s}_{md}") / m(f"pca_{s}_{md}") for s in ("u8", "rle") for md in ("full", "sample")}
        if not args.skip_old_route:
            out["old_route_over_hull_u8_sample"] = m("old_route_u8_sample") / m("hull_u8_sample")
            out["old_route_over_hull_u8_full"] = m("old_route_u8_sample") / m("hull_u8_full")
    f.status[0].sum().item()
    out["status_ok_fraction_last_call"] = float((f.status[0] == 0).float().mean().item())
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
