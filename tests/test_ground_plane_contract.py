"""CPU-only tests of the ground plane from depth (include/la3d.h "ground plane: RANSAC plane fit"; ``plane_select_batch``,
``plane_ransac_batch``, ``ground_planes``, ``PlaneFit``): the names on every layer, the argument blocks against the header, every
refusal of the two C entries with its code, its message and its rank in front of P = 0 (fake pointers: nothing here reaches a device),
the NumPy restatement on the synthetic scene, and the condition the generators owe the GPU tests - an eigen-gap of at least 1e-3 in
every fitted case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import la3d_oracle as O

from . import ground_plane_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2
NAN, INF = float("nan"), float("inf")


def test_names_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _build, _lib, depth_align

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    assert "ground plane: RANSAC plane fit" in hdr
    for fn in ("la3d_plane_select_batch", "la3d_plane_select_workspace_bytes", "la3d_plane_ransac_batch", "la3d_plane_ransac_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % fn, hdr) and fn in _lib.EXPORTS and hasattr(_lib.lib, fn), fn
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2          # additive
    assert re.search(r"#define LA3D_PLANE_MAX_TRIALS 1024\b", hdr) and _lib.PLANE_MAX_TRIALS == G.MAX_TRIALS == 1024
    assert re.search(r"#define LA3D_PLANE_SEGMENT 1024\b", hdr) and _lib.PLANE_SEGMENT == G.SEG
    assert any(s.endswith("la3d_plane.hip") for s in _build.SOURCES)
    assert all(any(h.endswith(n) for h in _build.HEADERS) for n in ("la3d_point.hpp", "la3d_draw.hpp"))
    for fn in ("plane_select_batch", "plane_ransac_batch", "ground_planes", "PlaneFit"):
        assert getattr(la, fn) is getattr(depth_align, fn) and fn in la.__all__, fn
    assert la.PlaneFit._fields == ("plane", "k_trial", "n_inliers", "best_trial", "rms", "status", "inliers")
    assert callable(la.PlaneFit.for_instances)
    # the shared pieces are shared, not restated
    csrc = os.path.join(ROOT, "labelany3d_amd", "csrc")
    for unit, header, name in (("la3d_plane.hip", "la3d_draw.hpp", "ar_subset_index"), ("la3d_align.hip", "la3d_draw.hpp", "ar_subset_index"),
                               ("la3d_plane.hip", "la3d_point.hpp", "cloud_point"), ("la3d_cloud.hip", "la3d_point.hpp", "cloud_point")):
        text = open(os.path.join(csrc, unit)).read()
        assert f'#include "{header}"' in text and not re.search(r"__device__[^;{]*\b%s\s*\(" % name, text), (unit, name)
    plane = open(os.path.join(csrc, "la3d_plane.hip")).read()
    assert "#pragma clang fp contract(off)" in plane and "asm" not in plane and "atomicAdd" not in plane


def _header_fields(name):
    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            base, star, names = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)", decl).groups()
            want += [(nm.strip(), C.c_void_p if star else ctype[base]) for nm in names.split(",")]
    return want


@pytest.mark.parametrize("name,size", [("la3d_plane_select_args", 112), ("la3d_plane_ransac_args", 152)])
def test_blocks_match_the_header(name, size):
    from labelany3d_amd import _lib

    block = {"la3d_plane_select_args": _lib.PlaneSelectArgs, "la3d_plane_ransac_args": _lib.PlaneRansacArgs}[name]
    want, got = _header_fields(name), list(block._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    off = 0
    for (n, t), (_, w) in zip(got, want):
        assert C.sizeof(t) == C.sizeof(w) and C.alignment(t) == C.alignment(w), n
        off = (off + C.alignment(w) - 1) // C.alignment(w) * C.alignment(w)
        assert getattr(block, n).offset == off, n
        off += C.sizeof(w)
    assert C.sizeof(block) == size == (off + 7) // 8 * 8


class Fake:
    """fake "device" memory, 64-byte aligned: every call below is refused, or has nothing to do, before any launch"""

    def __init__(self):
        self.buf = (C.c_char * 4096)()
        self.p = (C.addressof(self.buf) + 63) & ~63


def _select(f, **kw):
    from labelany3d_amd import _lib

    a = dict(struct_size=C.sizeof(_lib.PlaneSelectArgs), P=2, H=8, W=40, step=4, k_stride=0, near_depth=0.0, far_depth=INF, depth=f.p, K=f.p,
             candidates=None, cand_plane_stride=0, cand_width=0, reserved=0, points=f.p, pixel=f.p, counts=f.p, workspace=f.p, stream=None)
    a.update(kw)
    rc = _lib.lib.la3d_plane_select_batch(C.byref(_lib.PlaneSelectArgs(**a)))
    return rc, _lib.lib.la3d_last_error()


def _ransac(f, **kw):
    from labelany3d_amd import _lib

    a = dict(struct_size=C.sizeof(_lib.PlaneRansacArgs), P=2, n=64, points=f.p, counts=f.p, thr_abs=0.02, thr_rel=0.0, cos2_tilt=0.0,
             max_trials=16, min_inliers=0, subsets=None, seed=1, plane=f.p, k_trial=f.p, n_inliers=f.p, best_trial=f.p, rms=f.p, status=f.p,
             inliers=None, workspace=f.p, stream=None)
    a.update(kw)
    rc = _lib.lib.la3d_plane_ransac_batch(C.byref(_lib.PlaneRansacArgs(**a)))
    return rc, _lib.lib.la3d_last_error()


# (what is wrong, the code, a word of the message) - in the order the entry checks them
SELECT_REFUSALS = [
    (dict(struct_size=0), ARG, "struct_size"), (dict(struct_size=104), ARG, "struct_size"), (dict(struct_size=120), ARG, "struct_size"),
    (dict(H=-1), ARG, "negative P, H or W"), (dict(W=-1), ARG, "negative P, H or W"),
    (dict(step=0), ARG, "step must be at least 1"), (dict(step=-4), ARG, "step must be at least 1"),
    (dict(near_depth=NAN), ARG, "NaN"), (dict(far_depth=NAN), ARG, "NaN"),
    (dict(k_stride=5), ARG, "k_stride"), (dict(k_stride=-9), ARG, "k_stride"),
    (dict(reserved=1), ARG, "reserved"),
    (dict(candidates="p", cand_width=32), ARG, "multiple of 32 and >= W"), (dict(candidates="p", cand_width=72), ARG, "multiple of 32 and >= W"),
    (dict(candidates="p", cand_width=64, cand_plane_stride=-1), ARG, "plane stride >= 0"),
    (dict(depth="p+2"), ARG, "4-byte aligned"), (dict(pixel="p+2"), ARG, "4-byte aligned"), (dict(workspace="p+1"), ARG, "4-byte aligned"),
    (dict(candidates="p+2", cand_width=64), ARG, "4-byte aligned"),
    (dict(K="p+4"), ARG, "8-byte aligned"), (dict(points="p+4"), ARG, "8-byte aligned"), (dict(counts="p+4"), ARG, "8-byte aligned"),
    (dict(candidates="p", cand_width=64, cand_plane_stride=15), ARG, "below the words of a plane"),
]
SELECT_NULLS = ("depth", "K", "points", "pixel", "counts", "workspace")
SELECT_UNSUPPORTED = [(dict(H=32769, W=32768), "2^30"), (dict(P=65536), "65535")]

RANSAC_REFUSALS = [
    (dict(struct_size=0), ARG, "struct_size"), (dict(struct_size=144), ARG, "struct_size"), (dict(struct_size=160), ARG, "struct_size"),
    (dict(n=-1), ARG, "negative P or n"),
    (dict(max_trials=0), ARG, "max_trials must be at least 1"), (dict(max_trials=-5), ARG, "max_trials must be at least 1"),
    (dict(thr_abs=-0.01), ARG, "thr_abs and thr_rel"), (dict(thr_rel=-0.01), ARG, "thr_abs and thr_rel"),
    (dict(thr_abs=0.0, thr_rel=0.0), ARG, "not both zero"), (dict(thr_abs=NAN), ARG, "thr_abs and thr_rel"), (dict(thr_rel=INF), ARG, "thr_abs and thr_rel"),
    (dict(cos2_tilt=-0.1), ARG, "cos2_tilt outside [0, 1]"), (dict(cos2_tilt=1.0000001), ARG, "cos2_tilt outside [0, 1]"), (dict(cos2_tilt=NAN), ARG, "cos2_tilt"),
    (dict(min_inliers=-1), ARG, "min_inliers"),
    (dict(subsets="p+2"), ARG, "4-byte aligned"), (dict(k_trial="p+2"), ARG, "4-byte aligned"), (dict(n_inliers="p+1"), ARG, "4-byte aligned"),
    (dict(best_trial="p+2"), ARG, "4-byte aligned"), (dict(status="p+3"), ARG, "4-byte aligned"),
    (dict(points="p+4"), ARG, "8-byte aligned"), (dict(counts="p+4"), ARG, "8-byte aligned"), (dict(plane="p+4"), ARG, "8-byte aligned"),
    (dict(rms="p+4"), ARG, "8-byte aligned"),
    (dict(workspace="p+8"), ARG, "16-byte aligned"),
]
RANSAC_NULLS = ("points", "counts", "plane", "k_trial", "n_inliers", "best_trial", "rms", "status", "workspace")
RANSAC_UNSUPPORTED = [(dict(n=(1 << 24) + 1), "LA3D_PLANE_MAX_N"), (dict(max_trials=1025), "LA3D_PLANE_MAX_TRIALS"), (dict(P=65536), "65535")]


def _resolve(f, kw):
    return {k: (f.p + int(v[2:] or 0) if isinstance(v, str) else v) for k, v in kw.items()}


@pytest.mark.parametrize("entry", ["select", "ransac"])
def test_every_refusal_its_code_its_message_and_its_rank_before_P0(entry):
    from labelany3d_amd import _lib

    f = Fake()
    call, who, refusals, nulls, unsupported = ((_select, b"la3d_plane_select_batch: ", SELECT_REFUSALS, SELECT_NULLS, SELECT_UNSUPPORTED) if entry == "select"
                                               else (_ransac, b"la3d_plane_ransac_batch: ", RANSAC_REFUSALS, RANSAC_NULLS, RANSAC_UNSUPPORTED))
    fn = getattr(_lib.lib, "la3d_plane_%s_batch" % entry)
    assert fn(None) == ARG and _lib.lib.la3d_last_error().startswith(who)
    rc, msg = call(f, P=-1)
    assert rc == ARG and msg.startswith(who) and b"negative P" in msg
    for kw, code, word in refusals:
        for p0 in ({}, dict(P=0)):                                  # an argument error is refused whether or not there is work
            rc, msg = call(f, **dict(_resolve(f, kw), **p0))
            assert rc == code and msg.startswith(who) and word.encode() in msg, (kw, p0, rc, msg)
    for (kw_a, code_a, word_a), (kw_b, _, word_b) in zip(refusals, refusals[1:]):   # two errors at once: the one checked first answers
        if word_a != word_b and not set(kw_a) & set(kw_b):
            rc, msg = call(f, **_resolve(f, dict(kw_b, **kw_a)))
            assert rc == code_a and word_a.encode() in msg, (kw_a, kw_b, msg)
    for name in nulls:                                              # a NULL pointer counts only with work to do
        rc, msg = call(f, **{name: None})
        assert rc == ARG and b"NULL pointer with work to do" in msg, (name, rc, msg)
        assert call(f, P=0, **{name: None})[0] == 0, name
    for kw, word in unsupported:
        for p0 in ({}, dict(P=0)):
            if "P" in kw and p0:
                continue
            rc, msg = call(f, **dict(kw, **p0))
            assert rc == UNSUPPORTED and msg.startswith(who) and word.encode() in msg, (kw, p0, rc, msg)
    # the argument checks stand in front of the limits, the limits in front of "nothing to do"
    first = refusals[3][0]
    assert call(f, **dict(unsupported[0][0], **first))[0] == ARG
    assert call(f, P=0)[0] == 0 and call(f, P=0, **{n: None for n in nulls})[0] == 0
    if entry == "select":
        assert _lib.lib.la3d_plane_select_workspace_bytes(2, 480, 640, 4) == 2 * 5 * 4           # 19200 grid pixels: five chunks of 4096
        assert _lib.lib.la3d_plane_select_workspace_bytes(0, 480, 640, 4) == 16 == _lib.lib.la3d_plane_select_workspace_bytes(2, 480, 640, 0)
    else:
        assert call(f, n=0, points=None, P=0)[0] == 0
        small, large = (_lib.lib.la3d_plane_ransac_workspace_bytes(2, n, 256) for n in (1024, 1025))
        assert 0 < small < large and small % 16 == 0                                             # a second segment per frame
        assert _lib.lib.la3d_plane_ransac_workspace_bytes(2, 64, 1025) == 16 == _lib.lib.la3d_plane_ransac_workspace_bytes(0, 64, 8)


def test_the_restatement_recovers_the_plane_of_the_scene():
    s = G.scene()
    depth, mask = s["depth"], s["mask"]
    H, W = depth.shape
    assert (depth[:8] == G.FILL).all() and 300 < mask.sum() < 3000 and not mask[:, 0].any() and not mask[-1].any()
    pix = G.select_ref(depth, None, 4, 0.0, 100.0)
    assert 300 < len(pix) < (H // 4) * (W // 4) and (depth.reshape(-1)[pix] < 100).all()
    pts = O.depth_to_points(depth[None], s["K"]).reshape(-1, 3)[pix]
    sub = G._draw(np.random.default_rng(5), len(pix), 64)
    r = G.ransac_ref(pts, len(pix), sub, 0.005, 0.0, G.cos2(0.8))
    err, derr = G.angle(r["plane"][:3], s["normal"]), abs(r["plane"][3] - s["d"])
    print(f"scene: {len(pix)} samples, k_trial {r['k_trial']}, gap {r['gap']:.3f}, normal off by {err:.3e} rad, d {r['plane'][3]:.9f}")
    assert r["status"] == G.OK and r["gap"] >= 1e-3 and r["plane"][1] < 0
    assert err < 1e-4 and derr < 1e-3
    inl, rms = G.recount_ref(pts, r["plane"], 0.005, 0.0)
    assert inl.sum() >= r["k_trial"] * 0.98 and rms < 0.005
    assert not inl[mask.reshape(-1)[pix] & (np.abs(pts.dot(s["normal"]) + s["d"]) > 0.02)].any()      # nothing of the box above 2 cm


def test_the_scene_separates_a_grounded_fit_from_an_ungrounded_one():
    """the oracle's estimate_bbox on the box's own points: upright on the true plane its vertical dimension is the box's height to
    2 %; in the camera's tilted frame it overstates it by more than 10 %"""
    s = G.scene()
    pts = O.depth_to_points(s["depth"][None], s["K"])[s["mask"]]
    ground = np.array([*s["normal"], s["d"]])
    up = O.estimate_bbox(pts, None, ground, rand_ind=False)[2][1]
    tilted = O.estimate_bbox(pts, None, None, rand_ind=False)[2][1]
    print(f"box height {s['box_height']}: grounded {up:.4f}, ungrounded {tilted:.4f}")
    assert abs(up - s["box_height"]) <= 0.02 * s["box_height"]
    assert tilted > 1.10 * s["box_height"]


def test_every_fitted_case_of_the_generators_has_an_eigen_gap():
    """the condition the GPU tests' 1e-9 rad bound rests on: (l1 - l0) / l2 >= 1e-3 in EVERY status-0 case, none left out"""
    seen = {}
    for tag, cases in G.all_batches():
        cap = max(max(len(c["points"]) for c in cases), 1)
        for c in cases:
            r = G.expected(c, cap)
            seen.setdefault(c["name"], set()).add(r["status"])
            if r["status"] == G.OK:
                assert r["gap"] >= 1e-3, (tag, c["name"], r["gap"])
                assert r["k_trial"] >= 3 and 0 <= r["best_trial"] < len(c["subsets"])
    want = dict(clean={G.OK}, collinear={G.FAILED}, broken={G.BROKEN})
    for name, st in want.items():
        assert seen[name] == st, (name, seen[name])
    for name in ("wall", "repeated", "out_of_range", "non_finite", "ties"):
        assert G.OK in seen[name], name
    assert seen["tiny"] == {G.OK, G.TOO_FEW}


def test_the_generators_do_what_their_names_say():
    n, T = G.SEG + 1, 65
    w = G.wall(n, T, 7)
    with_prior, without = G.expected(w), G.expected(w, max_tilt=None)
    assert G.angle(with_prior["plane"][:3], G.NORMAL) < 1e-3 and abs(without["plane"][2]) > 0.9999     # floor / wall
    assert without["k_trial"] > with_prior["k_trial"]
    t = G.ties(n, T, 7)
    r = G.expected(t)
    twins = [i for i, s in enumerate(t["subsets"]) if (s == t["subsets"][r["best_trial"]]).all()]
    assert len(twins) >= 3 and r["best_trial"] == min(twins) == 0
    o = G.out_of_range(n, T, 7)
    assert ((o["subsets"] < 0) | (o["subsets"] >= o["count"])).any(axis=1).sum() >= T // 3 and o["count"] < n
    nf = G.non_finite(n, T, 7)
    assert (~np.isfinite(nf["points"][nf["subsets"][:, 0]])).any(axis=1).sum() >= T // 4
    rp = G.repeated(n, T, 7)
    assert (rp["subsets"][:, 0] == rp["subsets"][:, 1]).sum() >= T // 2 and G.expected(rp)["best_trial"] % 2 == 1
    assert G.expected(G.collinear(n, T, 7))["status"] == G.FAILED
    k = with_prior["k_trial"]
    assert G.expected(w, min_inliers=k)["status"] == G.OK and G.expected(w, min_inliers=k + 1)["status"] == G.FAILED     # min_inliers above the best k
