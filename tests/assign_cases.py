"""The NumPy restatement of the assignment on the device (include/la3d.h "assignment on the device") - SciPy's shortest augmenting
path solver (scipy.optimize.linear_sum_assignment, 1.15), step for step, ties included - and the cases its CPU and GPU tests share.
Costs are regenerated from seeds (``RandomState``), never stored; tests/golden/g21_assign.npz holds what SciPy returned for them."""
import os

import numpy as np

MAX_N, STAGE_MAX = 256, 2048          # LA3D_ASSIGN_MAX_N, LA3D_ASSIGN_STAGE_MAX
OK, INVALID, INFEASIBLE, TOO_LARGE, BROKEN = 0, 1, 2, 3, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_assign.npz")
INVALID_MESSAGE, INFEASIBLE_MESSAGE = "matrix contains invalid numeric entries", "cost matrix is infeasible"


class Invalid(ValueError):
    pass


class Infeasible(ValueError):
    pass


def _solve(cost, plain: bool):
    """nr <= nc, float64, no NaN / -inf -> col4row (nr,), or Infeasible.  ``plain``: the scan over ``remaining`` as SciPy writes it,
    one column at a time; else the same choice read in parallel (the least path cost; an unassigned column at the HIGHEST position,
    else the column at the LOWEST position)."""
    nr, nc = cost.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    path = np.full(nc, -1)
    for cur in range(nr):
        sp = np.full(nc, np.inf)
        SR, SC = np.zeros(nr, bool), np.zeros(nc, bool)
        remaining = np.arange(nc - 1, -1, -1)
        nrem, minv, i, sink = nc, 0.0, cur, -1
        while sink == -1:
            SR[i] = True
            if plain:
                lowest, index = np.inf, -1
                for t in range(nrem):
                    j = remaining[t]
                    r = ((minv + cost[i, j]) - u[i]) - v[j]
                    if r < sp[j]:
                        path[j] = i
                        sp[j] = r
                    if sp[j] < lowest or (sp[j] == lowest and row4col[j] == -1):
                        lowest, index = sp[j], t
            else:
                rem = remaining[:nrem]
                with np.errstate(invalid="ignore"):
                    r = ((minv + cost[i, rem]) - u[i]) - v[rem]
                better = r < sp[rem]
                path[rem[better]] = i
                sp[rem[better]] = r[better]
                lowest = sp[rem].min()
                tied = np.flatnonzero(sp[rem] == lowest)
                free = tied[row4col[rem[tied]] == -1]
                index = free[-1] if len(free) else tied[0]
            minv = lowest
            if minv == np.inf:
                raise Infeasible(INFEASIBLE_MESSAGE)
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            nrem -= 1
            remaining[index] = remaining[nrem]
        u[cur] += minv
        for i in np.flatnonzero(SR):
            if i != cur:
                u[i] += minv - sp[col4row[i]]
        v[SC] -= minv - sp[SC]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return col4row


def restatement(cost, maximize: bool = False, plain: bool = False) -> np.ndarray:
    """(na, nb) -> col_of_row (na,) int: the column SciPy matches each row with, -1 if none; Invalid / Infeasible where SciPy raises."""
    c = np.asarray(cost, np.float64)
    na, nb = c.shape
    if na == 0 or nb == 0:
        return np.full(na, -1)
    if maximize:
        c = -c
    if np.isnan(c).any() or np.isneginf(c).any():
        raise Invalid(INVALID_MESSAGE)
    out = np.full(na, -1)
    if na > nb:
        col4row = _solve(np.ascontiguousarray(c.T), plain)      # the solver's rows are B's
        out[col4row] = np.arange(nb)
    else:
        out[:] = _solve(c, plain)
    return out


def pairs_of(col_of_row):
    rows = np.flatnonzero(np.asarray(col_of_row) >= 0)
    return rows, np.asarray(col_of_row)[rows]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _both(shapes):
    out = []
    for s in shapes:
        for t in (s, s[::-1]):
            if t not in out:
                out.append(t)
    return out


# 0 x n, n x 0, 1 x 1, 1 x n, n x 1; 2 x 2; 7 x 9, 9 x 7; 63, 64, 65 columns; 64 x 65, 65 x 64; 129 x 128; both sides of the
# LDS-staging threshold (45 * 45 = 2025 <= 2048 < 46 * 46 = 2116; 8 x 256 = 2048 staged, 9 x 256 not); MAX_N and MAX_N + 1
SHAPES = _both([(0, 5), (1, 1), (1, 6), (2, 2), (7, 9), (5, 63), (5, 64), (5, 65), (64, 65), (129, 128), (45, 45), (46, 46),
                (8, MAX_N), (9, MAX_N), (MAX_N, MAX_N), (3, MAX_N + 1)])
FAMILIES = ("equal", "ints", "thirds", "iou", "uniform", "inf_feasible", "inf_infeasible", "nan", "neginf")
INTEGER_FAMILIES = ("equal", "ints")          # integer-valued: they also go through the int32 route


def make_cost(shape, family: str, seed: int) -> np.ndarray:
    na, nb = shape
    rs = np.random.RandomState(seed)
    if family == "equal":
        return np.ones((na, nb))
    if family == "ints":
        return rs.randint(0, 3, (na, nb)).astype(np.float64)
    if family == "thirds":
        return rs.randint(0, 4, (na, nb)) / 3.0
    if family == "iou":                        # IoU-like, 70 - 90 % zeros, negated (the cost hungarian_matching hands to SciPy)
        zeros = rs.uniform(0.7, 0.9)
        return -(rs.rand(na, nb) * (rs.rand(na, nb) >= zeros))
    c = rs.rand(na, nb)
    if family == "uniform" or c.size == 0:
        return c
    if family == "inf_feasible":               # +inf everywhere but on one full matching and a few more entries
        n = min(na, nb)
        keep = rs.rand(na, nb) < 0.3
        pa, pb = rs.permutation(na)[:n], rs.permutation(nb)[:n]
        keep[pa, pb] = True
        return np.where(keep, c, np.inf)
    if family == "inf_infeasible":             # a row of the smaller side without a finite entry, +inf sprinkled elsewhere
        c[rs.rand(na, nb) < 0.2] = np.inf
        if na <= nb:
            c[rs.randint(na), :] = np.inf
        else:
            c[:, rs.randint(nb)] = np.inf
        return c
    c[rs.randint(na), rs.randint(nb)] = np.nan if family == "nan" else -np.inf
    return c


def all_cases():
    """(name, shape, family, maximize, seed) of every case, in fixture order."""
    out = []
    for si, shape in enumerate(SHAPES):
        for fi, family in enumerate(FAMILIES):
            for maximize in (False, True):
                out.append((f"{shape[0]}x{shape[1]}-{family}-{'max' if maximize else 'min'}", shape, family, maximize, 1000 * si + fi))
    return out


def load_golden():
    """name -> (kind, col_of_row): kind 0 = SciPy returned (col_of_row int (na,)), 1 = it raised the invalid-entries error, 2 = the
    infeasible one."""
    z = np.load(GOLDEN)
    names, kinds, first, cols = [str(n) for n in z["names"]], z["kind"], z["first"], z["col_of_row"]
    return {n: (int(kinds[k]), cols[first[k]:first[k + 1]].astype(np.int64)) for k, n in enumerate(names)}


def expected_status(shape, kind: int) -> int:
    """the status the device gives a group whose matrix SciPy answered with ``kind``"""
    if shape[0] == 0 or shape[1] == 0:
        return OK
    if max(shape) > MAX_N:
        return TOO_LARGE
    return kind


def mixed_call(cases=None, empty_every: int = 3):
    """One multi-group call over the cases of one ``maximize`` value: the flat costs, offsets, counts and the case of every group (None:
    an empty group put between them - 0 x 0, 0 x 3 and 2 x 0 in turn)."""
    empties = [(0, 0), (0, 3), (2, 0)]
    costs, counts_a, counts_b, which = [], [], [], []
    for k, case in enumerate(cases):
        if k % empty_every == 0:
            e = empties[(k // empty_every) % 3]
            counts_a.append(e[0]); counts_b.append(e[1]); which.append(None)
        _, shape, family, _, seed = case
        costs.append(make_cost(shape, family, seed).reshape(-1))
        counts_a.append(shape[0]); counts_b.append(shape[1]); which.append(case)
    counts_a.append(0); counts_b.append(0); which.append(None)
    flat = np.concatenate(costs) if costs else np.zeros(0)
    sizes = np.asarray(counts_a, np.int64) * np.asarray(counts_b, np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return flat, offsets, np.asarray(counts_a, np.int32), np.asarray(counts_b, np.int32), which


# ---- mask matrices: what assign_overlap / match_masks read ---------------------------------------------------------------------------
MASK_FRAME = (96, 224)
MASK_COUNTS_A, MASK_COUNTS_B = [9, 3, 0, 7, 12], [8, 5, 2, 7, 4]


def mask_stacks():
    """boolean stacks A (sum of MASK_COUNTS_A, H, W) and B of one frame size: specials (all ones, empty, identical and nested pairs)
    among random blobs - many pairs without overlap, so ties decide"""
    from . import mask_overlap_cases as MC

    H, W = MASK_FRAME
    A = MC.with_specials(MC.blobs(301, sum(MASK_COUNTS_A), H, W))
    B = MC.blobs(302, sum(MASK_COUNTS_B), H, W)
    B[3] = A[2]
    return A, B


def frame_stacks():
    """per image of tests/frames_bits_cases.py (seven sizes, one image without rows): the masks of seed 0 as A, those of seed 1 as B"""
    from . import frames_bits_cases as FBC

    out = []
    ca, cb = FBC.make_case(0), FBC.make_case(1)
    for p, (h, w) in enumerate(FBC.SIZES):
        sa = [m for m, i in zip(ca["masks"], ca["img"]) if i == p]
        sb = [m for m, i in zip(cb["masks"], cb["img"]) if i == p]
        out.append((np.stack(sa) if sa else np.zeros((0, h, w), bool), np.stack(sb) if sb else np.zeros((0, h, w), bool)))
    return out


def mask_matrices(groups, kind: str = "iou"):
    """[(A_g, B_g)] boolean stacks -> per group (inter int64 (na, nb), ratio float64 (na, nb)): exact counts, one float64 division"""
    from . import mask_overlap_cases as MC

    out = []
    for A, B in groups:
        inter, aa, ab = MC.overlap_ref(A, B)
        out.append((inter, MC.ratio_ref(inter, aa, ab, kind)))
    return out


def split(stack, counts):
    first = np.concatenate([[0], np.cumsum(counts)])
    return [stack[first[g]:first[g + 1]] for g in range(len(counts))]


def mask_groups():
    A, B = mask_stacks()
    return list(zip(split(A, MASK_COUNTS_A), split(B, MASK_COUNTS_B)))
