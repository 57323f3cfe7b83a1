"""Round 6: the randomised differential campaign of the point-cloud entry (la3d_fit_points through labelany3d_amd.fit_points:
estimate_bbox for explicit clouds, reference src/util_3dbox.py:106-178 - what the reference's harness calls per mesh).

    python profiles/r06/fuzz_points.py [--cases 400] [--seed 0] [--workers 128] [--out profiles/r06/fuzz_points.txt]

The cases, the oracle, the GPU runs and the checkers live in oracle/campaigns/points.py (shared with
tests/test_gpu_differential.py, which runs a committed slice of the seeds); this script computes the CPU oracle on a pool of host
cores, runs every case through both yaw methods, every launch form and the scalar drop-in, and writes the record.
Nothing under /root/reference is read."""
import argparse
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.campaigns import points as PT  # noqa: E402

make_case, oracle_case = PT.make_case, PT.oracle_case   # (the campaign's cases under their old names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workers", type=int, default=min(128, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06", "fuzz_points.txt"))
    a = ap.parse_args()
    seeds = list(range(a.seed, a.seed + a.cases))
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = "1"
    t0 = time.time()
    with mp.get_context("spawn").Pool(a.workers) as pool:
        ref = dict(pool.imap_unordered(PT.oracle_case, seeds, chunksize=1))
    t_or = time.time() - t0

    import torch

    assert torch.cuda.is_available(), "the campaign needs the GPU"
    n_cloud = 0
    fails = []
    tally = PT.new_tally()
    t0 = time.time()
    for s in seeds:
        c = PT.make_case(s)
        n_cloud += c["B"]
        for method in PT.METHODS:
            for r in PT.runs_for(method):
                tag = f"seed {s} B={c['B']} {method} ground={'no' if c['ground'] is None else 'yes'} sample={c['sidx'] is not None} {r}"
                try:
                    got = PT.run_gpu(c, method, r)
                except Exception as e:   # noqa: BLE001
                    fails.append((tag, f"call failed: {e!r}")); continue
                fails += [(tag, m) for m in PT.check_run(c, ref[s][method], method, r, got, tally)]
        for method in PT.METHODS:
            st = ref[s][method][1]
            for n in PT.scalar_clouds(c):
                tally["n_scalar"] += 1
                tag = f"seed {s} cloud {n} ({len(c['clouds'][n])} rows) scalar drop-in {method}"
                fails += [(tag, m) for m in PT.check_scalar(c, ref[s][method], method, n, PT.run_scalar(c, method, n, st[n]))]
    t_gpu = time.time() - t0
    lines = [f"fuzz_points: {len(seeds)} cases (seeds {seeds[0]}..{seeds[-1]}), {n_cloud} clouds, both yaw methods, {len(PT.RUNS)} launches per case and method",
             f"oracle: {t_or:.0f} s on {a.workers} host cores; GPU runs + comparison: {t_gpu:.0f} s",
             f"records compared with the oracle: {tally['n_rec']} (+ {tally['n_tie']} PCA records with gap < 1e-9 - exact ties, no spread, or ill-conditioned for raw sums - held to status / counts; "
             f"{tally['n_hull_tied']} hull records whose minimum-area edge is tied within 1e-9 of the area, held to the area; {tally['n_hull_flat']} hull records of footprints without area (collinear within rounding: whether a hull exists is decided by the last bits), held to status / counts / height; {tally['n_cap']} hull clouds above 2048 valid rows: status 5)",
             f"scalar drop-in (la3d_estimate_bbox_host) calls compared: {tally['n_scalar']}",
             f"failures: {len(fails)}"]
    lines += [f"  FAIL {t}: {m}" for t, m in fails[:300]]
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
