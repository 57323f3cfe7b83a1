"""GPU tests of the frames call on 16-bit depth planes (include/la3d.h "images of different sizes in one call":
``la3d_fit_instances_frames_depth16``; ``pack_frames(dtype=...)`` -> ``PackedFrames16`` -> ``fit_instances_frames``) and of
``ScenePipeline(depth_dtype=...)``.

Inputs are the mixes of tests/test_gpu_frames.py (``make_mix``; its ``SIZES`` plus 61 x 75: pitches 224 - 640, heights that are no
multiple of 8, odd widths, a frame of fewer than 64 tiles, an image without instances), quantised with
``depth16_cases.quantise`` - never with the packer - in the three ``depth16_cases.VARIANTS``.  Two rules, both the suite's own:

* against the ORACLE run image by image on the up-converted, unpadded planes: records, yaw and 2-D boxes to rtol = atol = 1e-9,
  status / n_in / n_valid / filter statistics equal (``test_gpu_frames.check_strict``);
* against the FLOAT32 FRAMES CALL on ``upconvert(stored)`` of the same mix (``test_gpu_bits.same_engine``): status and
  ``aux[:, 1:3]`` equal, records to rtol = atol = 1e-12 - both calls are the instance engine's FRAMES form, and a 16-bit workgroup
  keeps the float32 lane-to-pixel mapping, so its sums are grouped as the float32 ones are.

The randomised sweep goes through degenerate masks and planes and uses the campaign's rule (oracle/campaigns/engines.py::check_run,
as tests/test_gpu_frames.py::test_randomised_sweep does)."""
import functools
import json

import numpy as np
import pytest

from oracle import la3d_oracle as O

from . import depth16_cases as DC
from .conftest import SCHED
from .test_gpu_bits import same_engine
from .test_gpu_frames import SIZES, check_strict, draws, frames_call, ground_rows, make_mix, np_, oracle_mix, shuffled, sweep_case
from .test_gpu_parity import assert_records, reference_axis_noise

pytestmark = pytest.mark.gpu

SIZES16 = SIZES + [(61, 75)]
VARIANTS = list(zip(DC.VARIANTS, DC.VARIANT_IDS))
KEYS = ("boxes", "status", "aux")


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


@functools.lru_cache(maxsize=None)
def base_mix(seed, poly, special=True):
    """(shared between the cases, never modified)"""
    return make_mix(seed, sizes=SIZES16, poly=poly, special=special)


def quantised(mix, variant):
    """(stored 16-bit planes, the mix on their up-converted planes: what the oracle and the float32 frames call get)"""
    dtype, scale, hole = variant
    stored = [DC.quantise(d, dtype, scale) for d in mix["depth"]]
    return stored, dict(mix, depth=[DC.upconvert(s, scale, hole) for s in stored])


def pack16(la, stored, variant):
    pf = la.pack_frames(stored, dtype=variant[0], scale=variant[1], zero_is_hole=variant[2])
    assert isinstance(pf, la.PackedFrames16) and pf.data.is_cuda
    return pf


def trio(res):
    return res["boxes"], res["status"], res["aux"]


# ------------------------------------------------------------------------------------------
# 1. one mixed call: both rules, every instantiation (run lengths / polygons x full mask / subsample), shuffled image_index
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
@pytest.mark.parametrize("grounded", [False, True], ids=["no-ground", "ground"])
@pytest.mark.parametrize("sample", [False, True], ids=["full", "subsample"])
@pytest.mark.parametrize("poly", [False, True], ids=["rle", "poly"])
def test_mixed_batch_both_rules(la, poly, sample, grounded, variant, vid):
    mix = base_mix(11 + poly, poly)
    assert len(set(mix["sizes"])) == 7 and not (mix["img"] == 2).any()
    B = len(mix["masks"])
    stored, up = quantised(mix, variant)
    ground = ground_rows(B, 5) if grounded else None          # (some rows NaN: "no ground" for those instances)
    sidx = draws(mix, 6) if sample else None
    ref = oracle_mix(up, ground, sidx)
    np.testing.assert_array_equal(ref[1], mix["expect"], err_msg="the oracle does not fit the chosen inputs as planned")   # on the CPU, first
    tag = f"{'poly' if poly else 'rle'} {'subsample' if sample else 'full'} {'ground' if grounded else 'no ground'} [{vid}]"
    pf16, pf32 = pack16(la, stored, variant), la.pack_frames(up["depth"])
    np.testing.assert_array_equal(pf16.table_host, pf32.table_host)
    got = frames_call(la, up, pf=pf16, ground=ground, sample_idx=sidx)
    check_strict(got, up, ref, tag)
    same_engine(trio(got), trio(frames_call(la, up, pf=pf32, ground=ground, sample_idx=sidx)), tag + " vs the float32 frames call")
    # the same instances in a shuffled order (image_index no longer sorted): every record follows its instance
    order = np.random.RandomState(3).permutation(B)
    perm = shuffled(up, 3)
    kw = dict(ground=None if ground is None else ground[order], sample_idx=None if sidx is None else sidx[order])
    got_s = frames_call(la, perm, pf=pf16, **kw)
    check_strict(got_s, perm, tuple(v[order] for v in ref), tag + " shuffled")
    same_engine(trio(got_s), trio(frames_call(la, perm, pf=pf32, **kw)), tag + " shuffled vs the float32 frames call")
    for k in KEYS:
        np.testing.assert_array_equal(got_s[k], got[k][order], err_msg=f"{tag}: {k} after the shuffle")


# ------------------------------------------------------------------------------------------
# 2. special values under the masks: the checked re-run and the two-pass form inside a frames workgroup
# ------------------------------------------------------------------------------------------
SPECIAL_SIZES = [(96, 224), (61, 75), (100, 214), (200, 320), (96, 224), (61, 75), (37, 53), (120, 160)]


def special_mix(variant):
    """eight images, one instance each (a centred rectangle: no other instance shares the plane), special words written into the
    STORED planes under the masks.  Returns (mix on the up-converted planes, stored planes, expected statuses, pixels dropped).
    Statuses 1 (nothing valid) and 3 (one valid point) are built here; status 4 cannot be reached through a depth value - an
    infinite depth under the mask is a hole, dropped as NaN is (tests/depth16_cases.py::special_checked) - so none is expected."""
    dtype, scale, hole = variant
    mix = make_mix(52, sizes=SPECIAL_SIZES, per_image=1, empty_image=-1, special=False)
    for m in mix["masks"]:
        h, w = m.shape
        m[:] = False
        m[h // 4:3 * h // 4, w // 4:3 * w // 4] = True
    stored = [DC.quantise(d, dtype, scale) for d in mix["depth"]]
    want, dropped = np.zeros(8, np.int32), np.zeros(8, np.int64)

    def under(n, k):
        r, c = np.argwhere(mix["masks"][n])[k]
        return int(r), int(c)

    if dtype == "f16":
        stored[0][under(0, 7)] = stored[0][under(0, 40)] = np.float16(np.nan); dropped[0] = 2        # NaN: dropped
        stored[1][under(1, 9)] = np.float16(np.inf); dropped[1] = 1                                     # +-inf: a hole, dropped like NaN
        stored[2][under(2, 11)] = np.float16(-2.0)                                                      # a negative depth is a point like any other
        stored[3][under(3, 5)] = np.float16(6e-8); stored[3][under(3, 6)] = np.float16(-0.0)            # smallest subnormal, -0
        stored[4][mix["masks"][4]] = np.float16(np.nan); want[4] = 1                                    # nothing valid
        keep = stored[5][under(5, 3)]
        stored[5][mix["masks"][5]] = np.float16(np.nan); stored[5][under(5, 3)] = keep; want[5] = 3     # one valid point
        stored[6][under(6, 13)] = np.float16(-np.inf); dropped[6] = 1
    else:
        stored[0][under(0, 7)] = stored[0][under(0, 40)] = 0; dropped[0] = 2 if hole else 0             # holes (or the valid depth 0.0)
        stored[1][under(1, 9)] = stored[1][under(1, 10)] = 65535
        stored[2][under(2, 11)] = 0; stored[2][under(2, 12)] = 65535; dropped[2] = 1 if hole else 0
        if hole:   # (without the flag a mask of depths 0.0 has no spread at all: the suite's documented don't-care, left out)
            stored[4][mix["masks"][4]] = 0; want[4] = 1
            keep = stored[5][under(5, 3)]
            stored[5][mix["masks"][5]] = 0; stored[5][under(5, 3)] = keep; want[5] = 3
    up = dict(mix, depth=[DC.upconvert(s, scale, hole) for s in stored])
    return up, stored, want, dropped


@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
def test_special_values_under_the_masks(la, variant, vid):
    up, stored, want, dropped = special_mix(variant)
    B = len(want)
    pf16, pf32 = pack16(la, stored, variant), la.pack_frames(up["depth"])
    for ground in (None, ground_rows(B, 7, some_nan=False)):
        tag = f"special values {'ground' if ground is not None else 'no ground'} [{vid}]"
        ref = oracle_mix(up, ground)
        np.testing.assert_array_equal(ref[1], want, err_msg="the oracle does not fit the chosen inputs as planned")
        got = frames_call(la, up, pf=pf16, ground=ground)
        np.testing.assert_array_equal(got["status"], want, err_msg=tag + ": expected statuses")
        check_strict(got, up, ref, tag)
        ok = want == 0
        np.testing.assert_array_equal(got["aux"][ok, 2] - got["aux"][ok, 1], dropped[ok], err_msg=tag + ": pixels dropped under the mask")
        same_engine(trio(got), trio(frames_call(la, up, pf=pf32, ground=ground)), tag + " vs the float32 frames call")


# ------------------------------------------------------------------------------------------
# 3. fused filter with statistics and proj, clamped to each instance's own frame: equal to the float32 frames call
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
@pytest.mark.parametrize("poly", [False, True], ids=["rle", "poly"])
def test_filter_stats_and_proj_equal_the_float32_call(la, poly, variant, vid):
    mix = base_mix(21 + poly, poly, special=False)
    stored, up = quantised(mix, variant)
    B = len(mix["masks"])
    pf16, pf32 = pack16(la, stored, variant), la.pack_frames(up["depth"])
    rec, st, yaw, nv = oracle_mix(up)
    assert (st == 0).all()
    for flt in (True, {"boundary_threshold": 3, "scale_threshold": 400}):
        b, a = (10, 100) if flt is True else (3, 400)
        stats = np.array([O.mask_stats(m, b) for m in mix["masks"]])
        keep = np.array([O.keep_instance(s, mix["sizes"][p][0], not poly, a) for s, p in zip(stats, mix["img"])])
        assert keep.any() and (~keep).any(), "the inputs should exercise both sides of the keep rule"
        got = frames_call(la, up, pf=pf16, filter=flt, proj=True)
        want = frames_call(la, up, pf=pf32, filter=flt, proj=True)
        for k in ("status", "stats", "aux", "boxes", "boxes2d"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}, filter {flt} [{vid}]")
        np.testing.assert_array_equal(got["stats"], stats, err_msg="filter statistics")
        expect = np.where(keep, st, 6).astype(np.int32)
        check_strict(got, up, (rec, st, yaw, nv), f"filter {flt} [{vid}]", expect=expect)
        ok = expect == 0
        want2d = np.stack([O.project_boxes(rec[i:i + 1], mix["K"][mix["img"][i]], (mix["sizes"][mix["img"][i]][1], mix["sizes"][mix["img"][i]][0]))[0]
                           for i in range(B)])
        np.testing.assert_allclose(got["boxes2d"][ok], want2d[ok], rtol=1e-9, atol=1e-9, err_msg="2-D boxes")
        assert np.isnan(got["boxes2d"][~ok]).all()
        clamp_w = np.asarray([mix["sizes"][p][1] for p in mix["img"]], float)
        clamp_h = np.asarray([mix["sizes"][p][0] for p in mix["img"]], float)
        assert (got["boxes2d"][ok, 6] <= clamp_w[ok]).all() and (got["boxes2d"][ok, 7] <= clamp_h[ok]).all()


# ------------------------------------------------------------------------------------------
# 4. an exactly sized buffer: the LAST plane has H % 8 != 0 and an odd width, an instance touches its last row and column
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
def test_exactly_sized_buffer_last_plane(la, variant, vid):
    mix = make_mix(44, sizes=[(96, 224), (100, 214), (61, 75)], per_image=3, empty_image=-1, special=False)
    last = [i for i in range(len(mix["masks"])) if mix["img"][i] == 2]
    m = mix["masks"][last[0]]
    m[:] = False
    m[38:61, 49:75] = True                                    # 598 px (sampled in subsample mode), the last row and the last image column
    mix["masks"][last[1]][60, :] = True                       # the whole last row
    stored, up = quantised(mix, variant)
    pf16, pf32 = pack16(la, stored, variant), la.pack_frames(up["depth"])
    t = pf16.table_host
    assert pf16.data.numel() == int(t["depth_offset"][-1]) + 61 * 96 and int(t["W"][-1]) == 96 and int(t["frame_width"][-1]) == 75
    for sidx in (None, draws(mix, 8)):
        tag = f"exact buffer {'subsample' if sidx is not None else 'full'} [{vid}]"
        ref = oracle_mix(up, None, sidx)
        assert (ref[1] == 0).all()
        got = frames_call(la, up, pf=pf16, sample_idx=sidx)
        check_strict(got, up, ref, tag)
        same_engine(trio(got), trio(frames_call(la, up, pf=pf32, sample_idx=sidx)), tag + " vs the float32 frames call")


# ------------------------------------------------------------------------------------------
# 5. contract breaks are answered per instance, on the device - with depth_offset counted in 16-bit elements
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
def test_contract_breaks_get_status_5(la, variant, vid):
    """Frame rows that break the contract (and image indices outside the table): their instances get status 5, a NaN record and
    aux = NaN, 0, NaN, NaN; every other instance of the call is fitted exactly as in the clean call.  Nothing is provoked: the kernel
    decides before it forms an address from a broken row (frame_geometry: off < 0, off & 3, the bounds).  The rows whose H, W or
    offset alignment is broken would - were they read all the same - still address words INSIDE the depth buffer (they belong to the
    small images at the front, the large ones lie behind them; asserted below); the negative offset of the second table has no such
    cover and needs none: it is refused by its sign."""
    import torch

    sizes = [(64, 96), (96, 224), (100, 214), (37, 53), (120, 160), (480, 640), (427, 640)]
    mix = make_mix(51, sizes=sizes, per_image=3, empty_image=-1, special=False)
    stored, up = quantised(mix, variant)
    pf = pack16(la, stored, variant)
    clean = frames_call(la, up, pf=pf, filter=True, proj=True)
    assert (clean["status"] != 5).all() and (clean["status"] == 0).any()

    def with_table(table):
        words = torch.as_tensor(np.ascontiguousarray(table).view(np.int32).reshape(len(sizes), 6).copy(), device="cuda")
        return pf._replace(table=words, table_host=table)

    def check(got, broken, tag):
        np.testing.assert_array_equal(got["status"][broken], 5, err_msg=tag)
        assert np.isnan(got["boxes"][broken]).all() and np.isnan(got["boxes2d"][broken]).all(), tag
        assert np.isnan(got["aux"][broken][:, [0, 2, 3]]).all() and (got["aux"][broken][:, 1] == 0).all(), tag
        for k in ("boxes", "status", "aux", "stats", "boxes2d"):
            np.testing.assert_array_equal(got[k][~broken], clean[k][~broken], err_msg=f"{tag}: {k} of the instances on conforming frames")

    table = pf.table_host.copy()
    table["depth_offset"][0] = 2                              # 4 bytes into the buffer: would pass a float rule, must not pass here
    table["depth_offset"][1] += 2
    table["H"][2] = pf.H + 8                                  # more rows than the bound of the call
    table["frame_width"][3] = table["W"][3] + 1               # more image columns than the pitch
    table["W"][4] = 48                                        # pitch not a multiple of 32 (frame_width 48 would fit it)
    table["frame_width"][4] = 48
    assert int(table["depth_offset"][2]) + (pf.H + 8) * int(table["W"][2]) <= pf.data.numel()
    img = mix["img"].copy()
    img[-1], img[-2] = len(sizes), -1                         # image_index outside [0, P): both ends
    got = frames_call(la, dict(up, img=img), pf=with_table(table), filter=True, proj=True)
    broken = np.isin(mix["img"], [0, 1, 2, 3, 4])
    broken[-1] = broken[-2] = True
    assert broken.sum() >= 10 and (~broken).sum() >= 4
    check(got, broken, f"first table [{vid}]")
    table2 = pf.table_host.copy()
    table2["depth_offset"][0] = -4                            # negative
    table2["frame_width"][1] = 0
    table2["H"][2] = 0
    table2["W"][3] = pf.W + 32                                # a pitch above the bound of the call
    table2["depth_offset"][4] += 6                            # 12 bytes: 4-byte aligned, not 8
    assert int(table2["depth_offset"][3]) + int(table2["H"][3]) * (pf.W + 32) <= pf.data.numel()
    got2 = frames_call(la, up, pf=with_table(table2), filter=True, proj=True)
    check(got2, np.isin(mix["img"], [0, 1, 2, 3, 4]), f"second table [{vid}]")


# ------------------------------------------------------------------------------------------
# 6. the launch order of a batch above 256 instances is invisible
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
def test_launch_order_is_invisible(la, variant, vid):
    mix = make_mix(91, sizes=[(96, 224), (61, 75)] * 3, per_image=50, empty_image=-1, special=False)
    B = len(mix["masks"])
    assert B == 300
    stored, up = quantised(mix, variant)
    pf16 = pack16(la, stored, variant)
    want = frames_call(la, up, pf=pf16)
    assert (want["status"] == 0).sum() >= B // 2
    areas = np.asarray([m.sum() for m in mix["masks"]], np.int32)
    for hint in (None, areas, np.random.RandomState(1).permutation(areas)):
        for order in (None, True, False):
            SCHED().launch_order = order
            try:
                got = frames_call(la, up, pf=pf16, area_hint=hint)
            finally:
                SCHED().launch_order = None
            for k in KEYS:
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}: hint {'no' if hint is None else 'yes'}, launch_order={order} [{vid}]")
    same_engine(trio(want), trio(frames_call(la, up, pf=la.pack_frames(up["depth"]), area_hint=areas)), f"B = 300 vs the float32 frames call [{vid}]")


# ------------------------------------------------------------------------------------------
# 7. stream ordering, pinned engines
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
def test_stream_ordering_and_pinned_engines(la, variant, vid):
    """the call is an enqueue on the caller's stream, ordered behind the upload of the planes; engine pins give way"""
    import torch

    mix = make_mix(71, sizes=[(96, 224), (64, 96), (100, 214), (200, 320)], per_image=4, empty_image=-1)
    stored, up = quantised(mix, variant)
    want = frames_call(la, up, pf=pack16(la, stored, variant))
    side = torch.cuda.Stream()
    got = frames_call(la, up, pf=pack16(la, stored, variant), stream=side)      # (packed - uploaded - on the current stream just before)
    side.synchronize()
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"side stream [{vid}]")
    pf = pack16(la, stored, variant)
    for engine in ("rows", "band", "split", "instance"):
        SCHED().engine = engine
        try:
            g = frames_call(la, up, pf=pf)
        finally:
            SCHED().engine = None
        for k in KEYS:
            np.testing.assert_array_equal(g[k], want[k], err_msg=f"pinned {engine} [{vid}]")


# ------------------------------------------------------------------------------------------
# 8. the scene pipeline
# ------------------------------------------------------------------------------------------
class CountSeededDraws:
    """``rng`` of a ScenePipeline whose draws do not depend on the ORDER the instances come in (the two modes batch the scenes
    differently): the 500 indices of a mask of N pixels come from a generator seeded with N."""

    def randint(self, lo, hi, n):
        return np.random.RandomState(int(hi)).randint(lo, hi, n)


def four_scenes(with_ground):
    from labelany3d_amd.fit_scenes import synthetic_scenes

    out = []
    for k, (h, w) in enumerate([(480, 640), (427, 640), (375, 500), (500, 333)]):
        sc, _ = synthetic_scenes(1, seed=100 + k, H=h, W=w, with_ground=with_ground)
        sc[0]["name"] = f"{h}x{w}-" + sc[0]["name"]
        out += sc
    return out


def run_pipeline(scenes, **kw):
    from labelany3d_amd.fit_scenes import ScenePipeline

    timings = {}
    pipe = ScenePipeline(batch_images=8, write=False, timings=timings, **kw)
    return {sc["name"]: recs.text for sc, recs in pipe.run(scenes)}, timings


@pytest.mark.parametrize("variant,vid", VARIANTS, ids=DC.VARIANT_IDS)
@pytest.mark.parametrize("two_phase", [False, True], ids=["one-phase", "grounds+subsample"])
def test_pipeline_depth_dtype(la, two_phase, variant, vid):
    dtype, scale, hole = variant
    base = four_scenes(with_ground=two_phase)
    stored = [dict(sc, depth=DC.quantise(sc["depth"], dtype, scale)) for sc in base]
    up = [dict(sc, depth=DC.upconvert(sc["depth"], scale, hole)) for sc in stored]
    kw = dict(subsample=True, rng=CountSeededDraws()) if two_phase else {}
    d16 = dict(depth_dtype=dtype, depth_scale=scale, depth_zero_is_hole=hole)
    mixed, t_mixed = run_pipeline(stored, mixed_frames=True, **d16, **kw)
    uniform, t_uniform = run_pipeline(stored, **d16, **kw)
    f32, t_f32 = run_pipeline(up, mixed_frames=True, **kw)
    assert sorted(mixed) == sorted(uniform) == sorted(f32) == sorted(sc["name"] for sc in base)
    n = 0
    for name in mixed:
        assert mixed[name] == uniform[name], f"{name}: 3dbbox.json differs between the mixed and the uniform mode [{vid}]"
        assert mixed[name] == f32[name], f"{name}: 3dbbox.json differs from the float32 pipeline on the up-converted planes [{vid}]"
        n += len(json.loads(mixed[name]))
    assert n >= 8
    assert t_mixed["images"] == t_uniform["images"] == t_f32["images"] == 4
    assert 0 < t_mixed["h2d_bytes"] < t_f32["h2d_bytes"] and 0 < t_uniform["h2d_bytes"] < t_f32["h2d_bytes"]
    # a scene of another dtype is refused by name
    wrong = [dict(stored[0], name="the-float32-scene", depth=up[0]["depth"])]
    with pytest.raises(ValueError, match="the-float32-scene"):
        run_pipeline(wrong, mixed_frames=True, **d16)


# ------------------------------------------------------------------------------------------
# 9. seeded randomised sweep over the campaign generators' shapes, on 16-bit planes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", range(4))
def test_randomised_sweep(la, chunk):
    """4 x 26 seeded cases of tests/test_gpu_frames.py::sweep_case (random size mixes, the campaign generators' mask shapes and depth
    planes - invalid pixels included -, polygons, ground rows, skewed cameras, subsample mode), the planes quantised in the variant
    of the chunk: against the oracle on the up-converted planes by the campaign's rule, and against the float32 frames call"""
    variant, vid = VARIANTS[chunk % len(VARIANTS)]
    rs = np.random.RandomState(7100 + chunk)
    n_ok = n_all = n_tie = 0
    for case in range(26):
        mix, ground, sidx = sweep_case(rs)
        stored, up = quantised(mix, variant)
        B = len(mix["masks"])
        tag = f"chunk {chunk} case {case} [{vid}]: B={B} sizes={mix['sizes']} poly={mix['segs'] is not None} ground={ground is not None} sample={sidx is not None}"
        rec, st, yaw, nv, kap = oracle_mix(up, ground, sidx, kappa=True)
        got = frames_call(la, up, pf=pack16(la, stored, variant), ground=ground, sample_idx=sidx)
        np.testing.assert_array_equal(got["status"], st, err_msg=tag + " status")
        ok = st == 0
        assert np.isnan(got["boxes"][~ok]).all(), tag
        np.testing.assert_array_equal(got["aux"][:, 2], [m.sum() for m in mix["masks"]], err_msg=tag + " n_in")
        np.testing.assert_array_equal(got["aux"][ok, 1], nv[ok], err_msg=tag + " n_valid")
        tie = ok & ~(got["aux"][:, 3] >= 1e-9)
        chk = ok & ~tie
        noise = reference_axis_noise(kap, got["aux"][:, 1], got["aux"][:, 3])
        assert_records(got["boxes"][chk], rec[chk], tag, gap=got["aux"][chk, 3], noise=noise[chk])
        same_engine(trio(got), trio(frames_call(la, up, ground=ground, sample_idx=sidx)), tag + " vs the float32 frames call")
        n_ok += int(chk.sum()); n_all += B; n_tie += int(tie.sum())
    print(f"sweep chunk {chunk} [{vid}]: {n_ok} of {n_all} instances compared record by record ({n_tie} exact ties)")
    assert 3 * n_ok >= n_all
