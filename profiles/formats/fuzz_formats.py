"""The randomised differential campaign over the mask, logit and label packers and the 16-bit depth packers, at scale.

    python profiles/formats/fuzz_formats.py [--cases 500] [--seed 90000] [--seeds a,b,...] [--workers 16] [--budget 0]
                                          [--out profiles/formats/fuzz_formats.txt]

The cases, the oracle, the GPU runs and the checker live in oracle/campaigns/formats.py (shared with tests/test_gpu_differential.py,
which runs a committed slice of the seeds, tests/campaign_slices.py::FORMAT_SEEDS); this script computes the CPU oracle on a pool of
host cores, runs every case through every entry of RUNS that applies, serially, and writes the record.  A call that FAILS (an
exception, not a mismatch) ends the campaign there: whatever made it fail is looked at before anything else runs on the device.
--budget SECONDS: no new case starts after that many seconds of GPU part - the record then says which contiguous prefix has run."""
import argparse
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.campaigns import formats as CL  # noqa: E402

THREAD_VARS = ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")


def _oracle(seed):
    return seed, CL.expected(CL.make_case(seed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=500)
    ap.add_argument("--seed", type=int, default=90000)
    ap.add_argument("--seeds", default="", help="comma-separated seeds instead of --seed / --cases")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--budget", type=float, default=0.0, help="seconds of GPU part after which no new case starts (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "formats", "fuzz_formats.txt"))
    a = ap.parse_args()
    seeds = [int(x) for x in a.seeds.split(",")] if a.seeds else list(range(a.seed, a.seed + a.cases))
    workers = max(1, min(16, a.workers))
    # one BLAS / OpenMP thread per oracle worker (the pool is the parallelism): a spawned worker loads NumPy while it imports this
    # module, so it has to find the setting in the environment it starts with; the parent's own values are back before the GPU part
    # begins.  The oracle of a chunk of 50 cases is computed ahead of its GPU part, so a budgeted run pays for no oracle it does not use
    saved = {v: os.environ.get(v) for v in THREAD_VARS}
    import torch

    assert torch.cuda.is_available(), "the campaign needs the GPU"
    tally = CL.new_tally()
    fails, stopped, done, t_or, t_gpu = [], None, 0, 0.0, 0.0
    os.environ.update({v: "1" for v in THREAD_VARS})
    try:
        pool = mp.get_context("spawn").Pool(workers)   # (the workers start here, with the setting)
    finally:
        for v, old in saved.items():
            os.environ.pop(v, None) if old is None else os.environ.__setitem__(v, old)
    with pool:
        for lo in range(0, len(seeds), 50):
            chunk = seeds[lo:lo + 50]
            t0 = time.time()
            refs = dict(pool.imap_unordered(_oracle, chunk, chunksize=1))
            t_or += time.time() - t0
            t0 = time.time()
            print(f"case {lo} of {len(seeds)} (seed {chunk[0]}), {len(fails)} failures, GPU part {t_gpu:.0f} s", flush=True)
            for s in chunk:
                if a.budget and t_gpu + time.time() - t0 > a.budget:
                    break
                c = CL.make_case(s)
                CL.tally_case(tally, c, refs[s])
                cache, default = {}, {}
                for r in CL.RUNS:
                    if not CL.applies(c, r):
                        continue
                    try:
                        got = CL.run_gpu(c, r, cache)
                    except Exception as e:   # noqa: BLE001
                        fails.append((s, r, f"call failed: {e!r}"))
                        stopped = (s, r)
                        break
                    CL.tally_call(tally, r)
                    fam = CL.family(r)
                    if fam is not None and r["entry"] != "fit" and fam not in default:
                        default[fam] = CL.decoded(c, r, got)
                    fails += [(s, r, m) for m in CL.check_run(c, refs[s], r, got, default.get(fam), tally=tally)]
                if stopped:
                    break
                done += 1
            t_gpu += time.time() - t0
            if stopped or done < lo + len(chunk):
                break
    lines = [f"fuzz_formats: {done} cases (seeds {seeds[0]}..{seeds[done - 1] if done else seeds[0]}) of the range {seeds[0]}..{seeds[-1]}"
             + ("" if done == len(seeds) else f": a contiguous prefix, seeds {seeds[done]}..{seeds[-1]} have NOT run"),
             f"oracle: {t_or:.0f} s on {workers} host cores; GPU runs + comparison: {t_gpu:.0f} s"]
    lines += CL.tally_lines(tally)
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
