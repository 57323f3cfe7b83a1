"""Round 6: a randomised differential campaign over every engine of the batched fit (the code paths new this round - eight-band
exchange, the one-launch row engine, the full-tile class of the instance engine - get the same inputs as the old ones).

    python profiles/r06/fuzz_engines.py [--cases 400] [--seed 0] [--seeds a,b,...] [--tiny] [--workers 128] [--out profiles/r06/fuzz_engines.txt]

The cases, the oracle, the GPU runs and the checker live in oracle/campaigns/engines.py (shared with
tests/test_gpu_differential.py, which runs a committed slice of the seeds); this script computes the CPU oracle on a pool of host
cores, runs every case through every entry of RUNS + ANN_RUNS and writes the record.  Nothing under /root/reference is read."""
import argparse
import functools
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.campaigns import engines as E  # noqa: E402

make_case, oracle_case = E.make_case, E.oracle_case   # (the campaign's cases under their old names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seeds", default="", help="comma-separated seeds instead of --seed / --cases")
    ap.add_argument("--tiny", action="store_true", help="frames of 1 ... 9 rows and 1 ... 40 columns (below one tile in either direction)")
    ap.add_argument("--workers", type=int, default=min(128, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06", "fuzz_engines.txt"))
    a = ap.parse_args()
    seeds = [int(x) for x in a.seeds.split(",")] if a.seeds else list(range(a.seed, a.seed + a.cases))
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):   # one thread per oracle worker (the pool is the parallelism)
        os.environ[v] = "1"
    t0 = time.time()
    with mp.get_context("spawn").Pool(a.workers) as pool:
        ref = {s: (r, st, nv, kp) for s, r, st, nv, kp in pool.imap_unordered(functools.partial(E.oracle_case, tiny=a.tiny), seeds, chunksize=1)}
    t_or = time.time() - t0

    import torch

    assert torch.cuda.is_available(), "the campaign needs the GPU"
    n_inst = n_poly = n_refused = 0
    fails = []
    all_runs = E.RUNS + E.ANN_RUNS
    tally = E.new_tally()
    t0 = time.time()
    for s in seeds:
        c = E.make_case(s, a.tiny)
        n_inst += c["B"]
        n_poly += c["segs"] is not None
        cache = {}
        for r in all_runs:
            if not E.applies(c, r):
                continue
            try:
                got = E.run_gpu(c, r, cache)
            except Exception as e:   # noqa: BLE001 - a campaign records every failure and goes on
                if E.documented_refusal(c, r, e):
                    n_refused += 1
                else:
                    fails.append((s, r, f"call failed: {e!r}"))
                continue
            fails += [(s, r, m) for m in E.check_run(c, ref[s], r, got, tally)]
    t_gpu = time.time() - t0
    lines = [f"fuzz_engines: {len(seeds)} cases (seeds {seeds[0]}..{seeds[-1]}), {n_inst} instances, {len(E.RUNS)} runs per case through the u8 entry + {len(E.ANN_RUNS)} through the annotation / extended entries (3 as run lengths, 3 as polygons for the {n_poly} polygon cases, 4 through la3d_fit_instances_ex with the 2-D boxes of the epilogue, an area hint and - run lengths / polygons - the fused filter: {tally['n_ex']} instances dropped by it)",
             f"oracle: {t_or:.0f} s on {a.workers} host cores; GPU runs + comparison: {t_gpu:.0f} s",
             f"records compared with the oracle: {tally['n_rec']} (+ {tally['n_tie']} exact ties held to status / counts only)",
             f"worst relative error of center / dims among records with an eigen-gap above 1e-4: {tally['worst']:.2e}",
             f"calls refused as documented (frames above 1 Mpx as run lengths / polygons / in subsample mode): {n_refused}",
             f"failures: {len(fails)}"]
    lines += [f"  compared under {k}: {tally['per_run'].get(k, 0)} (of them ill-conditioned for raw sums, kappa > 2^17, and resolved by the second moments pass: {tally['n_ill'].get(k, 0)})"
              for k in map(repr, all_runs)]
    lines += [f"  FAIL seed {s} {r}: {m}" for s, r, m in fails[:400]]
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
