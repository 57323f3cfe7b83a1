"""Round 6: randomised differential campaign of the path's other entries - everything either side of the box fit (unproject, run-length
decode, mask statistics, polygon rasterisation, both filter branches, box projection, IoU, masked ratio median, depth-alignment
selection / scatter, matcher unprojection).

    python profiles/r06/fuzz_aux.py [--cases 300] [--seed 0] [--out profiles/r06/fuzz_aux.txt]

The cases, the reference expressions, the GPU calls and the checker live in oracle/campaigns/aux.py (shared with
tests/test_gpu_differential.py, which runs a committed slice of the seeds); this script runs a range of seeds and writes the
record.  Nothing under /root/reference is read."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.campaigns import aux as X  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06", "fuzz_aux.txt"))
    a = ap.parse_args()

    import torch

    assert torch.cuda.is_available(), "the campaign needs the GPU"
    fails = []
    n = dict.fromkeys(X.COUNTS, 0)
    t0 = time.time()
    for seed in range(a.seed, a.seed + a.cases):
        tag = f"seed {seed}"
        try:
            c = X.make_case(seed)
            tag = f"seed {seed} {c['H']}x{c['W']}"
            fails += [(tag, m) for m in X.check(c, X.expected(c), X.run_gpu(c), n)]
        except Exception as e:   # noqa: BLE001 - a campaign records every failure and goes on
            fails.append((tag, f"raised {e!r}"))
    lines = [f"fuzz_aux: {a.cases} cases (seeds {a.seed}..{a.seed + a.cases - 1}) in {time.time() - t0:.0f} s",
             f"checked: {n['unproject']} unproject calls, {n['rle']} run-length masks decoded, {n['stats']} mask statistics rows, {n['keep']} filter decisions, "
             f"{n['poly']} polygon annotations rasterised, {n['project']} boxes projected, {n['iou']} IoU entries, {n['median']} masked ratio medians, {n['align']} depth-alignment selections / scatters, {n['matches']} match points unprojected",
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
