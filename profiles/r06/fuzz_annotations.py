"""Round 6: randomised differential campaign of the per-image annotation entries - the reference's real calling pattern
(read_bounding_boxes_segmentations, src/util.py:336-383, followed by the box fit of every kept instance).

    python profiles/r06/fuzz_annotations.py [--cases 600] [--seed 0] [--workers 128] [--out profiles/r06/fuzz_annotations.txt]

The cases, the oracle, the GPU calls and the checker live in oracle/campaigns/annotations.py (shared with
tests/test_gpu_differential.py, which runs a committed slice of the seeds); this script computes the CPU oracle on a pool of host
cores, runs every case through fit_annotations (GPU-resident and through the host entry) and fit_annotations_all with three
filters, and writes the record.  Nothing under /root/reference is read."""
import argparse
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.campaigns import annotations as A  # noqa: E402

make_case, oracle_case = A.make_case, A.oracle_case   # (the campaign's cases under their old names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=600)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workers", type=int, default=min(128, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06", "fuzz_annotations.txt"))
    a = ap.parse_args()
    seeds = list(range(a.seed, a.seed + a.cases))
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[v] = "1"
    t0 = time.time()
    with mp.get_context("spawn").Pool(a.workers) as pool:
        ref = dict(pool.imap_unordered(A.oracle_case, seeds, chunksize=1))
    t_or = time.time() - t0

    import torch

    assert torch.cuda.is_available(), "the campaign needs the GPU"
    fails = []
    n_ann = n_calls = n_dropped = 0
    tally = dict(n_rec=0)
    t0 = time.time()
    for s in seeds:
        c = A.make_case(s)
        keep = ref[s][2]
        n_ann += c["n"]
        n_dropped += int((~keep & np.array([m is not None for m in c["masks"]])).sum())
        for call in A.CALLS:
            tag = A.call_tag(c, call)
            try:
                got = A.run_gpu(c, call)
                n_calls += 1
            except Exception as e:   # noqa: BLE001
                fails.append((tag, f"raised {e!r}")); continue
            fails += [(tag, m) for m in A.check_call(c, ref[s], call, got, tally)]
    t_gpu = time.time() - t0
    lines = [f"fuzz_annotations: {len(seeds)} images (seeds {seeds[0]}..{seeds[-1]}), {n_ann} annotations, {n_calls} calls (fit_annotations on the GPU and through the host entry, fit_annotations_all with three filters)",
             f"oracle: {t_or:.0f} s on {a.workers} host cores; GPU runs + comparison: {t_gpu:.0f} s",
             f"every skip / keep decision compared ({n_dropped} annotations dropped by the rule with the case's thresholds); records compared with the oracle: {tally['n_rec']}",
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
