"""CPU-only tests of the assignment on the device (include/la3d.h "assignment on the device"): the names on every layer, the argument
blocks, the NumPy restatement of tests/assign_cases.py against what SciPy returned (tests/golden/g21_assign.npz) and against SciPy
itself where it imports, the refusals of the two C entries in their order (fake pointers: nothing here reaches a device) and the
Python argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import assign_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2


def test_names_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _build, _lib, assign

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    assert "assignment on the device" in hdr
    for fn in ("la3d_assign", "la3d_iou_matrix_groups"):
        assert re.search(r"\b%s\s*\(" % fn, hdr) and fn in _lib.EXPORTS and hasattr(_lib.lib, fn), fn
    for fn in ("assign_batch", "assign_overlap", "assign_plan", "match_masks", "match_boxes", "iou2d_groups", "Assignment", "AssignPlan", "BoxIou"):
        assert fn in la.__all__ and getattr(assign, fn) is getattr(la, fn), fn
    assert any(s.endswith("la3d_assign.hip") for s in _build.SOURCES)
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2     # additive
    for name, v in (("F64", 0), ("I32", 1), ("MAX_N", AC.MAX_N), ("STAGE_MAX", AC.STAGE_MAX), ("OK", AC.OK), ("INVALID", AC.INVALID),
                    ("INFEASIBLE", AC.INFEASIBLE), ("TOO_LARGE", AC.TOO_LARGE), ("BROKEN", AC.BROKEN)):
        assert re.search(r"#define LA3D_ASSIGN_%s %d\b" % (name, v), hdr) and getattr(_lib, "ASSIGN_" + name) == v, name
    assert AC.MAX_N >= 256 and AC.MAX_N % 64 == 0 and assign.MAX_N == AC.MAX_N
    # the blocks: size and the offset of every field, from the header's order and the C rules for x86-64 / amdgcn
    want = {"struct_size": 0, "G": 4, "cost": 8, "cost_dtype": 16, "reserved0": 20, "ncost": 24, "offsets": 32, "row_offsets_a": 40,
            "row_offsets_b": 48, "rows_a": 56, "rows_b": 64, "maximize": 72, "reserved1": 76, "col_of_row": 80, "row_of_col": 88, "status": 96,
            "stream": 104}
    assert C.sizeof(_lib.AssignArgs) == 112 and {n: getattr(_lib.AssignArgs, n).offset for n, _ in _lib.AssignArgs._fields_} == want
    want = {"struct_size": 0, "G": 4, "boxes_a": 8, "boxes_b": 16, "rows_a": 24, "rows_b": 32, "row_offsets_a": 40, "row_offsets_b": 48,
            "offsets": 56, "npairs": 64, "out": 72, "stream": 80}
    assert C.sizeof(_lib.IouGroupsArgs) == 88 and {n: getattr(_lib.IouGroupsArgs, n).offset for n, _ in _lib.IouGroupsArgs._fields_} == want
    for block, fields in (("la3d_assign_args", _lib.AssignArgs._fields_), ("la3d_iou_groups_args", _lib.IouGroupsArgs._fields_)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (block, block), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [n for n, _ in fields], block                             # the header's order is the ctypes order


def answer(cost, maximize, plain=False):
    try:
        return AC.OK, AC.restatement(cost, maximize, plain)
    except AC.Invalid:
        return AC.INVALID, np.full(cost.shape[0], -1)
    except AC.Infeasible:
        return AC.INFEASIBLE, np.full(cost.shape[0], -1)


def test_the_fixture_holds_every_case():
    gold = AC.load_golden()
    cases = AC.all_cases()
    assert len(cases) == len(AC.SHAPES) * len(AC.FAMILIES) * 2 and len({c[0] for c in cases}) == len(cases)
    assert all(c[0] in gold for c in cases)
    for want in ((0, 5), (5, 0), (1, 1), (1, 6), (6, 1), (2, 2), (7, 9), (9, 7), (64, 65), (65, 64), (129, 128), (AC.MAX_N, AC.MAX_N),
                 (3, AC.MAX_N + 1), (AC.MAX_N + 1, 3)):
        assert want in AC.SHAPES, want
    assert {63, 64, 65} <= {s[1] for s in AC.SHAPES}
    sizes = sorted(min(s) * max(s) for s in AC.SHAPES)                    # both sides of the staging threshold, and the threshold itself
    assert AC.STAGE_MAX in sizes and any(AC.STAGE_MAX - 64 < s < AC.STAGE_MAX for s in sizes) and any(AC.STAGE_MAX < s < AC.STAGE_MAX + 128 for s in sizes)
    kinds = np.asarray([gold[c[0]][0] for c in cases])
    assert (kinds == AC.OK).sum() > 200 and (kinds == AC.INVALID).sum() > 50 and (kinds == AC.INFEASIBLE).sum() > 10
    assert str(np.load(AC.GOLDEN)["scipy"]) in open(os.path.join(ROOT, "tests", "golden", "VERSIONS_assign.txt")).read()
    assert os.path.getsize(AC.GOLDEN) < 400 * 1024


def test_restatement_equals_the_fixture_on_every_case():
    gold = AC.load_golden()
    for name, shape, family, maximize, seed in AC.all_cases():
        kind, col = answer(AC.make_cost(shape, family, seed), maximize)
        assert kind == gold[name][0] and np.array_equal(col, gold[name][1]), name
    for tag, groups in (("masks", AC.mask_groups()), ("frames", AC.frame_stacks())):
        for g, (inter, ratio) in enumerate(AC.mask_matrices(groups)):
            for what, m in (("iou", ratio), ("inter", inter)):
                kind, col = answer(m, True)
                assert kind == gold[f"{tag}-{g}-{what}"][0] == AC.OK and np.array_equal(col, gold[f"{tag}-{g}-{what}"][1]), (tag, g, what)


def test_the_plain_scan_and_its_parallel_reading_agree():
    """SciPy's scan over ``remaining``, one column at a time, against the choice the kernel makes (least cost; an unassigned column at
    the highest position, else the lowest position) - on the shapes a Python loop can afford"""
    for name, shape, family, maximize, seed in AC.all_cases():
        if shape[0] * shape[1] <= 64 * 65:
            cost = AC.make_cost(shape, family, seed)
            a, b = answer(cost, maximize, plain=True), answer(cost, maximize)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]), name


def test_restatement_equals_live_scipy():
    so = pytest.importorskip("scipy.optimize")
    rs = np.random.RandomState(7)
    for k in range(400):
        na, nb = rs.randint(1, 14, 2)
        fam = k % 4
        c = (rs.randint(0, 3, (na, nb)).astype(float) if fam == 0 else rs.rand(na, nb) * (rs.rand(na, nb) > 0.7) if fam == 1 else rs.rand(na, nb)
             if fam == 2 else rs.randint(0, 4, (na, nb)) / 3.0)
        if k % 5 == 0:
            c[rs.rand(na, nb) < 0.3] = np.inf
        maximize = bool(k % 3 == 0)
        try:
            rows, cols = so.linear_sum_assignment(c, maximize=maximize)
            want = np.full(na, -1)
            want[rows] = cols
            got = AC.restatement(c, maximize)
            assert np.array_equal(got, want), k
            r, cc = AC.pairs_of(got)
            assert np.array_equal(r, rows) and np.array_equal(cc, cols)
        except ValueError as e:
            if isinstance(e, (AC.Invalid, AC.Infeasible)):
                raise AssertionError(f"case {k}: SciPy returned, the restatement raised {e}") from None
            with pytest.raises(ValueError, match=str(e)):
                AC.restatement(c, maximize)


class Fake:
    """fake "device" memory, 64-byte aligned: every call below is refused, or has nothing to do, before any launch"""

    def __init__(self):
        self.buf = (C.c_char * 16384)()
        self.p = (C.addressof(self.buf) + 63) & ~63


def test_assign_entry_refuses_in_order_before_any_launch():
    from labelany3d_amd import _lib

    f = Fake()

    def call(**kw):
        a = dict(struct_size=C.sizeof(_lib.AssignArgs), G=1, cost=f.p, cost_dtype=_lib.ASSIGN_F64, ncost=9, offsets=f.p + 1024,
                 row_offsets_a=f.p + 2048, row_offsets_b=f.p + 3072, rows_a=3, rows_b=3, maximize=0, col_of_row=f.p + 4096,
                 row_of_col=f.p + 5120, status=f.p + 6144)
        a.update(kw)
        return _lib.lib.la3d_assign(C.byref(_lib.AssignArgs(**a))), _lib.lib.la3d_last_error()

    assert _lib.lib.la3d_assign(None) == ARG and b"la3d_assign: NULL block" in _lib.lib.la3d_last_error()
    # each refusal with every later one also present: the order is the header's
    later = dict(G=-1, cost_dtype=7, maximize=2, offsets=None, cost=f.p + 4)
    rc, msg = call(struct_size=104, **later)
    assert rc == ARG and b"struct_size" in msg
    for name in ("G", "rows_a", "rows_b", "ncost"):
        rc, msg = call(**dict(dict(later, G=1), **{name: -1}))
        assert rc == ARG and b"negative" in msg, name
    del later["G"]
    rc, msg = call(**later)
    assert rc == ARG and b"cost_dtype" in msg
    rc, msg = call(**dict(later, cost_dtype=_lib.ASSIGN_I32))
    assert rc == ARG and b"maximize must be 0 or 1" in msg
    assert call(maximize=-1)[0] == ARG
    assert call(G=0, offsets=None, cost=f.p + 4, status=None)[0] == 0              # nothing to do: success whatever the pointers
    for name in ("cost", "offsets", "row_offsets_a", "row_offsets_b", "col_of_row", "row_of_col", "status"):
        rc, msg = call(**{name: None, "row_offsets_a" if name != "row_offsets_a" else "status": f.p + 2050})
        assert rc == ARG and b"NULL" in msg, name
    assert call(cost=f.p + 4)[0] == ARG and b"aligned" in call(cost=f.p + 4)[1]           # 8 bytes for float64
    assert call(cost=f.p + 2, cost_dtype=_lib.ASSIGN_I32)[0] == ARG                         # 4 bytes for int32
    assert call(offsets=f.p + 1024 + 4)[0] == ARG
    for name, at in (("row_offsets_a", 2048), ("row_offsets_b", 3072), ("col_of_row", 4096), ("row_of_col", 5120), ("status", 6144)):
        assert call(**{name: f.p + at + 2})[0] == ARG, name


def test_iou_groups_entry_refuses_before_any_launch():
    from labelany3d_amd import _lib

    f = Fake()

    def call(**kw):
        a = dict(struct_size=C.sizeof(_lib.IouGroupsArgs), G=1, boxes_a=f.p, boxes_b=f.p + 1024, rows_a=3, rows_b=3, row_offsets_a=f.p + 2048,
                 row_offsets_b=f.p + 3072, offsets=f.p + 4096, npairs=9, out=f.p + 5120)
        a.update(kw)
        return _lib.lib.la3d_iou_matrix_groups(C.byref(_lib.IouGroupsArgs(**a)))

    assert _lib.lib.la3d_iou_matrix_groups(None) == ARG and b"la3d_iou_matrix_groups" in _lib.lib.la3d_last_error()
    assert call(struct_size=80) == ARG
    for name in ("G", "rows_a", "rows_b", "npairs"):
        assert call(**{name: -1}) == ARG, name
    assert call(G=0, out=None) == 0 and call(npairs=0, boxes_a=None, out=None) == 0
    for name in ("boxes_a", "boxes_b", "row_offsets_a", "row_offsets_b", "offsets", "out"):
        assert call(**{name: None}) == ARG, name
    for name, at in (("boxes_a", 0), ("boxes_b", 1024), ("offsets", 4096), ("out", 5120)):
        assert call(**{name: f.p + at + 4}) == ARG, name
    assert call(row_offsets_a=f.p + 2048 + 2) == ARG and call(row_offsets_b=f.p + 3072 + 2) == ARG


def test_python_argument_errors_come_before_any_device_work():
    import torch

    import labelany3d_amd as la

    host = torch.zeros(12, dtype=torch.float64)                           # on the host: never reaches a device
    with pytest.raises(ValueError, match="assign_batch: cost must be float64 or int32"):
        la.assign_batch(host.float(), None, [3], [4])
    with pytest.raises(ValueError, match="assign_batch: cost must be float64 or int32"):
        la.assign_batch(np.zeros(12, np.float32), None, [3], [4])
    with pytest.raises(ValueError, match="assign_batch: a cost tensor must live on the GPU"):
        la.assign_batch(host, None, [3], [4])
    c = np.zeros(12)
    with pytest.raises(ValueError, match="assign_batch: maximize must be True or False"):
        la.assign_batch(c, None, [3], [4], maximize=1)
    with pytest.raises(ValueError, match="assign_batch: counts_a and counts_b are required"):
        la.assign_batch(c, None, None, [4])
    with pytest.raises(ValueError, match="assign_batch: counts_a must be a host sequence of ints"):
        la.assign_batch(c, None, torch.tensor([3]), [4])
    with pytest.raises(ValueError, match="assign_batch: counts_b must not hold a negative"):
        la.assign_batch(c, None, [3], [-4])
    with pytest.raises(ValueError, match="assign_batch: counts_a has 1 groups and counts_b 2"):
        la.assign_batch(c, None, [3], [2, 2])
    with pytest.raises(ValueError, match=r"assign_batch: offsets must hold G \+ 1 = 2 ints"):
        la.assign_batch(c, [0, 6, 12], [3], [4])
    with pytest.raises(ValueError, match="assign_batch: offsets must be a host sequence"):
        la.assign_batch(c, torch.tensor([0, 12]), [3], [4])
    with pytest.raises(ValueError, match="assign_batch: a group's matrix lies outside the 12 elements"):
        la.assign_batch(c, [1, 13], [3], [4])
    with pytest.raises(ValueError, match="assign_batch: a group's matrix lies outside"):
        la.assign_batch(c, [-1, 11], [3], [4])
    with pytest.raises(ValueError, match="assign_batch: a group's matrix lies outside"):
        la.assign_batch(c, None, [3, 1], [4, 1])
    with pytest.raises(ValueError, match="assign_batch: plan must be the AssignPlan"):
        la.assign_batch(c, None, [3], [4], plan=object())
    with pytest.raises(ValueError, match="assign_plan: counts_a has 2 groups"):
        la.assign_plan(None, [3, 1], [4])
    # assign_overlap
    ov = la.MaskOverlap(torch.zeros(12, dtype=torch.int32), None, torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32),
                        np.asarray([0, 12]), np.asarray([3], np.int32), np.asarray([4], np.int32))
    with pytest.raises(ValueError, match="assign_overlap: overlap must be the MaskOverlap"):
        la.assign_overlap((ov.inter, ov.offsets))
    with pytest.raises(ValueError, match="assign_overlap: what must be 'iou' or 'inter'"):
        la.assign_overlap(ov, what="iom")
    with pytest.raises(ValueError, match="assign_overlap: maximize must be True or False"):
        la.assign_overlap(ov, maximize=None)
    with pytest.raises(ValueError, match="assign_overlap: this overlap was computed without iou"):
        la.assign_overlap(ov)
    with pytest.raises(ValueError, match="assign_overlap: plan must be the AssignPlan"):
        la.assign_overlap(ov, what="inter", plan=(1, 2))
    # match_masks
    from . import mask_overlap_cases as MC

    def mb(n, H=33):
        return la.MaskBits(torch.zeros((n, MC.plane_words(H, 64)), dtype=torch.int32), H, 64, 47)

    with pytest.raises(ValueError, match="match_masks: kind must be"):
        la.match_masks(mb(3), mb(4), kind="inter")
    with pytest.raises(ValueError, match="match_masks: b is required"):
        la.match_masks(mb(3), None)
    for bad in ("0.5", True, float("nan")):
        with pytest.raises(ValueError, match="match_masks: min_value must be a number or None"):
            la.match_masks(mb(3), mb(4), min_value=bad)
    with pytest.raises(ValueError, match="match_masks: a and b state different frames"):
        la.match_masks(mb(3), mb(4, H=34))
    with pytest.raises(ValueError, match="match_masks: counts_a sums to 2"):
        la.match_masks(mb(3), mb(4), counts_a=[1, 1], counts_b=[2, 2])
    with pytest.raises(ValueError, match="match_masks: the planes must be a MaskBits or a FrameBits"):
        la.match_masks(np.zeros((3, 8, 8), bool), mb(4))
    # match_boxes / iou2d_groups
    b3, b4 = np.zeros((3, 4)), np.zeros((4, 4))
    for fn, who in ((la.match_boxes, "match_boxes"), (la.iou2d_groups, "iou2d_groups")):
        with pytest.raises(ValueError, match=who + r": boxes0 must be \(n, 4\) xyxy boxes"):
            fn(np.zeros((3, 5)), b4)
        with pytest.raises(ValueError, match=who + r": boxes1 must be \(n, 4\)"):
            fn(b3, np.zeros(8))
        with pytest.raises(ValueError, match=who + ": counts0 sums to 2"):
            fn(b3, b4, [1, 1], [2, 2])
        with pytest.raises(ValueError, match=who + ": counts1 sums to 5"):
            fn(b3, b4, [1, 2], [2, 3])
        with pytest.raises(ValueError, match=who + ": counts0 has 2 groups and counts1 1"):
            fn(b3, b4, [1, 2], [4])


def test_assignment_reads_its_tables_on_the_host():
    """``pairs`` and ``raise_for_status`` on host tensors (what the device would have written): SciPy's return and SciPy's messages"""
    import torch

    import labelany3d_amd as la

    a = la.Assignment(torch.tensor([2, -1, 0, -1, -1, 1], dtype=torch.int32), torch.tensor([2, -1, 0, -1, 2, -1], dtype=torch.int32),
                      torch.tensor([0, 0, 0], dtype=torch.int32), np.asarray([3, 0, 3], np.int32), np.asarray([3, 1, 3], np.int32))
    assert [x.tolist() for x in a.pairs(0)] == [[0, 2], [2, 0]] and a.pairs(0)[0].dtype == np.int64
    assert [x.tolist() for x in a.pairs(1)] == [[], []] and [x.tolist() for x in a.pairs(2)] == [[2], [1]]
    a.raise_for_status()
    with pytest.raises(ValueError, match="pairs: group 3 outside"):
        a.pairs(3)
    for status, msg in ((AC.INVALID, AC.INVALID_MESSAGE), (AC.INFEASIBLE, AC.INFEASIBLE_MESSAGE), (AC.TOO_LARGE, "more than 256 rows or columns"),
                        (AC.BROKEN, "tables of the call are broken")):
        bad = la.Assignment(a.col_of_row, a.row_of_col, torch.tensor([0, 0, status], dtype=torch.int32), a.counts_a, a.counts_b)
        with pytest.raises(ValueError, match=msg):
            bad.raise_for_status()


def test_combine_refuses_an_unknown_matching(tmp_path):
    import labelany3d_amd.combine as combine

    with pytest.raises(ValueError, match="combine_coco_results: matching must be 'host' or 'device', not 'bogus'"):
        combine.combine_coco_results(str(tmp_path), "val", str(tmp_path / "out.json"), matching="bogus")
