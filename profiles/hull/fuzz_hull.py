"""The randomised differential campaign over the convex-hull yaw of the depth + mask fit, at scale.

    python profiles/hull/fuzz_hull.py [--cases 500] [--seed 70000] [--seeds a,b,...] [--workers 16] [--budget 0]
                                      [--out profiles/hull/fuzz_hull.txt]

The cases, the coverage rule, the oracle, the GPU runs and the checker live in oracle/campaigns/hull.py (shared with
tests/test_gpu_differential.py, which runs a committed slice of the seeds, tests/campaign_slices.py::HULL_SEEDS); this script computes
the CPU oracle on a pool of host cores, runs every case through every entry of RUNS and writes the record.  A call that FAILS (an
exception, not a mismatch) ends the campaign there: whatever made it fail is looked at before anything else runs on the device.
--budget SECONDS: no new case starts after that many seconds of GPU part - the record then says which contiguous prefix has run."""
import argparse
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.campaigns import hull as HU  # noqa: E402


THREAD_VARS = ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")


def _oracle(seed):
    return seed, HU.Ref(HU.make_case(seed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=500)
    ap.add_argument("--seed", type=int, default=70000)
    ap.add_argument("--seeds", default="", help="comma-separated seeds instead of --seed / --cases")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--budget", type=float, default=0.0, help="seconds of GPU part after which no new case starts (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hull", "fuzz_hull.txt"))
    a = ap.parse_args()
    seeds = [int(x) for x in a.seeds.split(",")] if a.seeds else list(range(a.seed, a.seed + a.cases))
    workers = max(1, min(16, a.workers))
    t0 = time.time()
    # one BLAS / OpenMP thread per oracle worker (the pool is the parallelism).  A spawned worker loads NumPy while it imports this
    # module, before any initializer could run, so it has to find the setting in the environment it starts with; the parent's own
    # values are back before the GPU part of the script begins
    saved = {v: os.environ.get(v) for v in THREAD_VARS}
    os.environ.update({v: "1" for v in THREAD_VARS})
    try:
        with mp.get_context("spawn").Pool(workers) as pool:
            refs = dict(pool.imap_unordered(_oracle, seeds, chunksize=1))
    finally:
        for v, old in saved.items():
            os.environ.pop(v) if old is None else os.environ.__setitem__(v, old)
    t_or = time.time() - t0

    import torch

    assert torch.cuda.is_available(), "the campaign needs the GPU"
    tally = HU.new_tally()
    fails, n_inst, n_calls, stopped, done = [], 0, 0, None, 0
    t0 = time.time()
    for i, s in enumerate(seeds):
        if a.budget and time.time() - t0 > a.budget:
            break
        if i % 25 == 0:
            print(f"case {i} of {len(seeds)} (seed {s}), {len(fails)} failures, {time.time() - t0:.0f} s", flush=True)
        c = HU.make_case(s)
        n_inst += c["B"]
        cache, default = {}, None
        for r in HU.RUNS:
            if not HU.applies(c, r):
                continue
            try:
                got = HU.run_gpu(c, r, cache)
            except Exception as e:   # noqa: BLE001
                fails.append((s, r, f"call failed: {e!r}"))
                stopped = (s, r)
                break
            n_calls += 1
            if not r:
                default = got
            if r in HU.PINS and default is not None:
                fails += [(s, r, m) for m in HU.check_pin(default, got)]
            fails += [(s, r, m) for m in HU.check_run(c, refs[s], r, got, tally)]
        if stopped:
            break
        done += 1
    t_gpu = time.time() - t0
    lines = [f"fuzz_hull: {done} cases (seeds {seeds[0]}..{seeds[done - 1] if done else seeds[0]}) of the range {seeds[0]}..{seeds[-1]}"
             + ("" if done == len(seeds) else f": a contiguous prefix, seeds {seeds[done]}..{seeds[-1]} have NOT run") + f", {n_inst} instances, {n_calls} calls ({len(HU.SOURCES)} mask sources + {len(HU.PINS)} pins "
             f"that hull calls ignore, compared byte for byte with the default run)",
             f"oracle: {t_or:.0f} s on {workers} host cores; GPU runs + comparison: {t_gpu:.0f} s"]
    lines += HU.tally_lines(tally)
    if stopped:
        lines.append(f"STOPPED at seed {stopped[0]} {stopped[1]}: the call failed")
    lines.append(f"failures: {len(fails)}")
    lines += [f"  FAIL seed {s} {r}: {m}" for s, r, m in fails[:400]]
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
