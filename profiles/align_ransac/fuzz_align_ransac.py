"""The randomised differential campaign over the batched RANSAC scale fit, at scale.

    python profiles/align_ransac/fuzz_align_ransac.py [--cases 500] [--seed 100000] [--seeds a,b,...] [--budget 0] [--no-slice]
                                                      [--out profiles/align_ransac/fuzz_align_ransac.txt]

The cases, the oracle, the GPU runs and the checker live in oracle/campaigns/align_ransac.py (shared with
tests/test_gpu_differential.py, which runs a committed slice of the seeds, tests/campaign_slices.py::ALIGN_RANSAC_SEEDS).  One process,
serial: the CPU oracle of a case, then every entry of RUNS that applies to it.  A call that FAILS (an exception, not a mismatch) ends
the campaign there - nothing is tried again: whatever made it fail is looked at before anything else runs on the device.
--budget SECONDS: no new case starts after that many seconds - the record then says which contiguous prefix has run.  After the range
the committed slice runs once more in its groups of six, for the seconds a group takes in the suite."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.campaigns import align_ransac as AR  # noqa: E402
from tests import campaign_slices as S  # noqa: E402


def run_case(s, tally, per_run, fails):
    """(seconds of oracle, seconds of GPU runs + comparison, the run that failed or None)"""
    t0 = time.time()
    c = AR.make_case(s)
    want = AR.expected(c)
    AR.tally_case(tally, c, want)
    t1 = time.time()
    cache, default = {}, None
    for r in AR.RUNS:
        if not AR.applies(c, r):
            continue
        try:
            got = AR.run_gpu(c, r, cache)
        except Exception as e:   # noqa: BLE001
            fails.append((s, r, f"call failed: {e!r}"))
            return t1 - t0, time.time() - t1, r
        tally["calls"] += 1
        per_run[repr(r)] += 1
        if not r:
            default = got
        fails += [(s, r, m) for m in AR.check_run(c, want, r, got, default, tally)]
    return t1 - t0, time.time() - t1, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=500)
    ap.add_argument("--seed", type=int, default=100000)
    ap.add_argument("--seeds", default="", help="comma-separated seeds instead of --seed / --cases")
    ap.add_argument("--budget", type=float, default=0.0, help="seconds after which no new case starts (0: none)")
    ap.add_argument("--no-slice", action="store_true", help="do not time the committed slice after the range")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_ransac", "fuzz_align_ransac.txt"))
    a = ap.parse_args()
    seeds = [int(x) for x in a.seeds.split(",")] if a.seeds else list(range(a.seed, a.seed + a.cases))
    import torch

    assert torch.cuda.is_available(), "the campaign needs the GPU"
    tally = AR.new_tally()
    per_run = {repr(r): 0 for r in AR.RUNS}
    fails, stopped, done, t_or, t_gpu, start = [], None, 0, 0.0, 0.0, time.time()
    for i, s in enumerate(seeds):
        if a.budget and time.time() - start > a.budget:
            break
        if i % 50 == 0:
            print(f"case {i} of {len(seeds)} (seed {s}), {len(fails)} failures, oracle {t_or:.0f} s, GPU part {t_gpu:.0f} s", flush=True)
        o, g, bad = run_case(s, tally, per_run, fails)
        t_or, t_gpu = t_or + o, t_gpu + g
        if bad is not None:
            stopped = (s, bad)
            break
        done += 1
    lines = [f"fuzz_align_ransac: {done} cases (seeds {seeds[0]}..{seeds[done - 1] if done else seeds[0]}) of the range {seeds[0]}..{seeds[-1]}"
             + ("" if done == len(seeds) else f": a contiguous prefix, seeds {seeds[done]}..{seeds[-1]} have NOT run"),
             f"device: {torch.cuda.get_device_name(0)}; oracle: {t_or:.0f} s on one host core; GPU runs + comparison (with the oracle of the "
             f"device-drawn fits): {t_gpu:.0f} s"]
    lines += AR.tally_lines(tally)
    lines += [f"  calls of run {k}: {v}" for k, v in per_run.items()]
    if stopped:
        lines.append(f"STOPPED at seed {stopped[0]} {stopped[1]}: the call failed")
    elif not a.no_slice:
        lines.append(f"the committed slice ({len(S.ALIGN_RANSAC_SEEDS)} seeds) in its groups of six - seconds of a group: oracle + GPU runs and comparison")
        st, sp, sf = AR.new_tally(), {repr(r): 0 for r in AR.RUNS}, []
        for lo in range(0, len(S.ALIGN_RANSAC_SEEDS), 6):
            group, o, g, bad = S.ALIGN_RANSAC_SEEDS[lo:lo + 6], 0.0, 0.0, None
            for s in group:
                o1, g1, bad = run_case(s, st, sp, sf)
                o, g = o + o1, g + g1
                if bad is not None:
                    break
            lines.append(f"  group {group[0]}: {o:.2f} + {g:.2f} s")
            if bad is not None:
                lines.append(f"STOPPED in the slice at seed {s} {bad}: the call failed")
                break
        lines += ["  " + ln for ln in AR.tally_lines(st)]
        fails += sf
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
