"""Depth alignment with the estimator on the GPU (align_depth_batch: select -> RANSAC scale fit -> apply) against the route it
replaces (align_depth frame by frame: select on the GPU, scikit-learn's RANSACRegressor on the host, apply on the GPU), for P = 1, 16,
64 frames of 640 x 480 with a mask and 30 % outliers.

    python profiles/align_ransac/measure_align_ransac.py [--out FILE] [--no-host] [--host-frames N] [--only-fit P]

Per P: warm-up, then REPS timed calls through the wrappers, each on the next of SETS input sets (no call re-reads its predecessor's
bytes); median with min - max in microseconds per call (wall clock around a synchronised call).  The host route is timed on the same
frames, once per frame (it takes seconds per frame).  --only-fit P: REPS calls of ransac_scale_batch alone on P frames - for a kernel
trace, whose per-kernel times give the candidates pass's achieved bytes/s against its byte model (printed here).
"""
import argparse
import io
import json
import os
import statistics
import sys
import time
from contextlib import redirect_stdout

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from labelany3d_amd import align_depth, align_depth_batch, align_select_batch, ransac_scale_batch  # noqa: E402

H, W, T = 480, 640, 100


def make_frames(P, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    rel = torch.rand((P, H, W), generator=g, device=dev) * 3.5 + 0.5
    met = 3.7 * rel + 0.05 * torch.randn((P, H, W), generator=g, device=dev)
    out = torch.rand((P, H, W), generator=g, device=dev) < 0.3
    met = torch.where(out, torch.rand((P, H, W), generator=g, device=dev) * 29.9 + 0.1, met)
    mask = torch.rand((P, H, W), generator=g, device=dev) < 0.8
    return rel.contiguous(), met.contiguous(), mask.contiguous()


def timed(fn, sets, reps, warmup):
    for i in range(warmup):
        fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    us = []
    for i in range(reps):
        s = sets[(warmup + i) % len(sets)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(s)
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us), reps=reps)


def byte_model(P, counts):
    """Bytes the candidates pass moves: every sample once (x and y), the T slopes per workgroup, one partial row of T trials per
    workgroup (k, min, max: 4 bytes each; three float64 sums)."""
    n = int(sum(counts))
    segs = int(sum((c + 4095) // 4096 for c in counts))
    return n * 8 + segs * T * 4 + segs * T * 36


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-frames", type=int, default=64, help="frames of the largest batch the host route is timed on")
    ap.add_argument("--only-fit", type=int, default=0, metavar="P")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.only_fit:
        P = a.only_fit
        rel, met, mask = make_frames(P, 1, dev)
        ro, mo, cnt = align_select_batch(rel, met, mask, 400.0)
        for i in range(a.reps):
            ransac_scale_batch(ro, mo, cnt, 0.2, T, seed=i)
        torch.cuda.synchronize()
        counts = cnt.cpu().tolist()
        print(json.dumps(dict(only_fit=P, calls=a.reps, samples=int(sum(counts)), candidates_bytes_per_call=byte_model(P, counts),
                              candidate_tests_per_call=int(sum(counts)) * T)))
        return
    rows = []
    for P in (1, 16, 64):
        nsets = 4 if P < 64 else 3
        sets = [make_frames(P, 100 * P + s, dev) for s in range(nsets)]
        full = timed(lambda s: align_depth_batch(s[0], s[1], s[2], 0.2, 400.0, seed=7), sets, a.reps, 3)
        sel = [align_select_batch(s[0], s[1], s[2], 400.0) for s in sets]
        fit = timed(lambda s: ransac_scale_batch(s[0], s[1], s[2], 0.2, T, seed=7), sel, a.reps, 3)
        _, res = align_depth_batch(*sets[0], 0.2, 400.0, seed=7)
        row = dict(P=P, device_route=full, fit_only=fit, statuses=sorted(set(res.status.cpu().tolist())),
                   coef_first=float(res.coef[0]), n_trials_first=int(res.n_trials[0]))
        if not a.no_host and P <= a.host_frames:
            rel, met, mask = sets[0]
            np.random.seed(5)
            per_frame = []
            for p_ in range(P):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with redirect_stdout(io.StringIO()):
                    out = align_depth(rel[p_], met[p_], mask[p_], 0.2, 400.0)
                torch.cuda.synchronize()
                per_frame.append((time.perf_counter() - t0) * 1e6)
            row["host_route"] = dict(total_us=sum(per_frame), per_frame_median_us=statistics.median(per_frame),
                                     per_frame_min_us=min(per_frame), per_frame_max_us=max(per_frame), frames=P)
            row["ratio_host_over_device"] = sum(per_frame) / full["median_us"]
            row["coef_host_last"] = float((out[mask[P - 1]] / rel[P - 1][mask[P - 1]]).median())
        rows.append(row)
        print(json.dumps(row), flush=True)
        del sets, sel
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
