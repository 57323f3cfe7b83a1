"""Writes tests/golden/g21_assign.npz: what ``scipy.optimize.linear_sum_assignment`` itself returns - or which of its two errors it
raises - for every case of tests/assign_cases.py (costs regenerated from seeds, not stored) and for the mask matrices of its two mask
cases (maximize on the IoU and on the intersection counts).  Only integers are written: per case the column of every row (-1: none)
and the kind of answer.  Needs SciPy.  The committed fixture was written with python 3.10.12, numpy 2.2.6, scipy 1.15.3 (the
fixture's ``scipy`` entry holds the last; tests/golden/VERSIONS_assign.txt records all three).

    python tests/golden/make_golden_assign.py
"""
import os
import sys

import numpy as np
import scipy
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import assign_cases as AC  # noqa: E402


def scipy_answer(cost, maximize):
    """-> (kind, col_of_row)"""
    try:
        rows, cols = linear_sum_assignment(cost, maximize=maximize)
    except ValueError as e:
        kind = {AC.INVALID_MESSAGE: AC.INVALID, AC.INFEASIBLE_MESSAGE: AC.INFEASIBLE}[str(e)]
        return kind, np.full(cost.shape[0], -1)
    assert (np.diff(rows) > 0).all()
    out = np.full(cost.shape[0], -1)
    out[rows] = cols
    return AC.OK, out


def main():
    names, kinds, cols = [], [], []
    for name, shape, family, maximize, seed in AC.all_cases():
        kind, col = scipy_answer(AC.make_cost(shape, family, seed), maximize)
        names.append(name); kinds.append(kind); cols.append(col)
    for tag, groups in (("masks", AC.mask_groups()), ("frames", AC.frame_stacks())):
        for g, (inter, ratio) in enumerate(AC.mask_matrices(groups)):
            for what, m in (("iou", ratio), ("inter", inter.astype(np.float64))):
                kind, col = scipy_answer(m, True)
                names.append(f"{tag}-{g}-{what}"); kinds.append(kind); cols.append(col)
    first = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    flat = np.concatenate(cols)
    assert flat.max() < 2 ** 15
    np.savez_compressed(os.path.join(HERE, "g21_assign.npz"), names=np.asarray(names), kind=np.asarray(kinds, np.int8), first=first,
                        col_of_row=flat.astype(np.int16), scipy=np.asarray(scipy.__version__))
    print(len(names), "cases,", np.bincount(kinds).tolist(), "by kind,", os.path.getsize(os.path.join(HERE, "g21_assign.npz")), "bytes")


if __name__ == "__main__":
    main()
