"""GPU slices of the differential campaigns (oracle/campaigns/, driven at scale by profiles/r06/fuzz_*.py): fixed seed lists
(tests/campaign_slices.py) through the campaigns' own GPU runners and checkers, against the CPU oracle computed here, serially.

  engines       every entry of RUNS (default dispatch, every pinned engine, both two-pass builds, launch order off) and ANN_RUNS (run
                lengths, polygons, la3d_fit_instances_ex with the 2-D box epilogue, an area hint and the fused filter) for 45 regular
                and 40 tiny-frame cases
  points        both yaw methods, every launch form of RUNS and the scalar drop-in, 40 cases
  annotations   fit_annotations (GPU-resident and through the host entry) and fit_annotations_all with three filters, 40 images
  hull          the convex-hull yaw of the depth + mask fit (oracle/campaigns/hull.py): every mask source, the pins hull calls ignore
                (the same bytes as the default run), full-mask and subsample mode, 60 cases
  clouds        the instance point clouds (oracle/campaigns/clouds.py): u8 and bit planes, float32 output, every 16-bit kind, the
                frames form, a short capacity and the C entry in place, with and without sample_idx, 48 cases
  formats       the format converters in front of the fit (oracle/campaigns/formats.py): the mask, logit and label packers of one
                frame size and of mixed sizes, host and device layouts, out= buffers, the unpacker, the bit-plane statistics, both
                16-bit depth packers and the fit on the planes they wrote, 45 cases; the fit leg of the whole slice once more on its own, held to the share of
                records that must be compared
  align_ransac  the batched RANSAC scale fit (oracle/campaigns/align_ransac.py): explicit subsets batched, every frame alone, the same
                call twice, unaligned buffers, the device draw and the fit on it, select -> fit -> apply on depth frames, 48 cases
  aux           unproject, decoders, mask statistics, filters, consumers, depth statistics, matcher, 40 cases
A case fails with the campaign's own message, which names its seed."""
import numpy as np
import pytest

from oracle.campaigns import align_ransac as AR
from oracle.campaigns import annotations as A
from oracle.campaigns import aux as X
from oracle.campaigns import clouds as CL
from oracle.campaigns import engines as E
from oracle.campaigns import formats as FM
from oracle.campaigns import hull as HU
from oracle.campaigns import points as PT
from tests import campaign_slices as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd  # noqa: F401


def _groups(seeds, n):
    return [seeds[i:i + n] for i in range(0, len(seeds), n)]


def _report(fails):
    return f"{len(fails)} failures:\n" + "\n".join(fails[:20])


@pytest.mark.parametrize("tiny,seeds", [(False, g) for g in _groups(S.ENGINE_SEEDS, 5)] + [(True, g) for g in _groups(S.ENGINE_TINY_SEEDS, 10)],
                         ids=lambda v: str(v[0]) if isinstance(v, list) else ("tiny" if v else "regular"))
def test_engine_campaign_slice(gpu, tiny, seeds):
    fails = []
    for s in seeds:
        c = E.make_case(s, tiny)
        ref = E.oracle_case(s, tiny)[1:]
        cache = {}
        for r in E.RUNS + E.ANN_RUNS:
            if not E.applies(c, r):
                continue
            try:
                got = E.run_gpu(c, r, cache)
            except Exception as e:   # noqa: BLE001 - every failure of the slice is reported, not only the first
                if not E.documented_refusal(c, r, e):
                    fails.append(f"seed {s} {r}: call failed: {e!r}")
                continue
            fails += [f"seed {s} {r}: {m}" for m in E.check_run(c, ref, r, got)]
    assert not fails, _report(fails)


@pytest.mark.parametrize("seeds", _groups(S.POINT_SEEDS, 10), ids=lambda v: str(v[0]))
def test_point_campaign_slice(gpu, seeds):
    fails = []
    for s in seeds:
        c = PT.make_case(s)
        ref = PT.oracle_case(s)[1]
        for method in PT.METHODS:
            for r in PT.runs_for(method):
                try:
                    got = PT.run_gpu(c, method, r)
                except Exception as e:   # noqa: BLE001
                    fails.append(f"seed {s} {method} {r}: call failed: {e!r}"); continue
                fails += [f"seed {s} {method} {r}: {m}" for m in PT.check_run(c, ref[method], method, r, got)]
            for n in PT.scalar_clouds(c):
                got = PT.run_scalar(c, method, n, ref[method][1][n])
                fails += [f"seed {s} cloud {n} scalar drop-in {method}: {m}" for m in PT.check_scalar(c, ref[method], method, n, got)]
    assert not fails, _report(fails)


@pytest.mark.parametrize("seeds", _groups(S.ANNOTATION_SEEDS, 10), ids=lambda v: str(v[0]))
def test_annotation_campaign_slice(gpu, seeds):
    fails = []
    for s in seeds:
        c = A.make_case(s)
        ref = A.oracle_case(s)[1]
        for call in A.CALLS:
            try:
                got = A.run_gpu(c, call)
            except Exception as e:   # noqa: BLE001
                fails.append(f"{A.call_tag(c, call)}: raised {e!r}"); continue
            fails += [f"{A.call_tag(c, call)}: {m}" for m in A.check_call(c, ref, call, got)]
    assert not fails, _report(fails)


@pytest.mark.parametrize("seeds", _groups(S.AUX_SEEDS, 10), ids=lambda v: str(v[0]))
def test_aux_campaign_slice(gpu, seeds):
    fails = []
    for s in seeds:
        c = X.make_case(s)
        fails += [f"seed {s} {c['H']}x{c['W']}: {m}" for m in X.check(c, X.expected(c), X.run_gpu(c))]
    assert not fails, _report(fails)


@pytest.mark.parametrize("seeds", _groups(S.HULL_SEEDS, 6), ids=lambda v: str(v[0]))
def test_hull_campaign_slice(gpu, seeds):
    """method="convex_hull": status against the oracle and the documented coverage rule (HU.covered), every fitted record by its
    class (decided / tied / flat or fallback, from the oracle alone); the pinned runs equal the default run byte for byte."""
    fails = []
    tally = HU.new_tally()
    for s in seeds:
        c = HU.make_case(s)
        ref = HU.oracle_case(s)
        cache, default = {}, None
        for r in HU.RUNS:
            if not HU.applies(c, r):
                continue
            try:
                got = HU.run_gpu(c, r, cache)
            except Exception as e:   # noqa: BLE001 - every failure of the slice is reported, not only the first
                fails.append(f"seed {s} {r}: call failed: {e!r}")
                continue
            if not r:
                default = got
            if r in HU.PINS:
                fails += [f"seed {s} {r}: {m}" for m in (HU.check_pin(default, got) if default is not None else ["no default run to compare with"])]
            fails += [f"seed {s} {r}: {m}" for m in HU.check_run(c, ref, r, got, tally)]
    print("\n".join(HU.tally_lines(tally)))
    assert not fails, _report(fails)


@pytest.mark.parametrize("seeds", _groups(S.CLOUD_SEEDS, 6), ids=lambda v: str(v[0]))
def test_cloud_campaign_slice(gpu, seeds):
    """instance_points / instance_points_frames / the C entry: counts, offsets, status, pixels and every row (the unproject row of its
    pixel) exactly, points within 1e-13 of the oracle, the runs among each other.  A call that raises ends the group's GPU work."""
    fails = []
    tally = CL.new_tally()
    for s in seeds:
        c = CL.make_case(s)
        want = CL.oracle_case(s)
        CL.tally_case(tally, c, want)
        cache, default = {}, None
        for r in CL.RUNS:
            if not CL.applies(c, r):
                continue
            try:
                got = CL.run_gpu(c, r, cache)
            except Exception as e:   # noqa: BLE001 - whatever made the call fail is looked at before anything else runs on the device
                print("\n".join(CL.tally_lines(tally)))
                pytest.fail(_report(fails + [f"seed {s} {r}: call failed, nothing more was run: {e!r}"]))
            tally["calls"] += 1
            if not r:
                default = got
            fails += [f"seed {s} {r}: {m}" for m in CL.check_run(c, want, r, got, default)]
    print("\n".join(CL.tally_lines(tally)))
    assert not fails, _report(fails)


@pytest.mark.parametrize("seeds", _groups(S.FORMAT_SEEDS, 6), ids=lambda v: str(v[0]))
def test_format_campaign_slice(gpu, seeds):
    """The packers, the unpacker, the statistics and the 16-bit depth packers: every word, padding bit, area, offset and sentinel
    exactly, the runs among each other, and the fit on the packed planes by the engines campaign's rule.  A call that raises ends the
    group's GPU work."""
    fails = []
    tally = FM.new_tally()
    for s in seeds:
        c = FM.make_case(s)
        want = FM.oracle_case(s)
        FM.tally_case(tally, c, want)
        cache, default = {}, {}
        for r in FM.RUNS:
            if not FM.applies(c, r):
                continue
            try:
                got = FM.run_gpu(c, r, cache)
            except Exception as e:   # noqa: BLE001 - whatever made the call fail is looked at before anything else runs on the device
                print("\n".join(FM.tally_lines(tally)))
                pytest.fail(_report(fails + [f"seed {s} {r}: call failed, nothing more was run: {e!r}"]))
            FM.tally_call(tally, r)
            fam = FM.family(r)
            if fam is not None and fam not in default:
                default[fam] = FM.decoded(c, r, got)
            fails += [f"seed {s} {r}: {m}" for m in FM.check_run(c, want, r, got, default.get(fam), tally=tally)]
    print("\n".join(FM.tally_lines(tally)))
    assert not fails, _report(fails)


def test_format_slice_fit_leg_compares_a_third(gpu):
    """The fit leg of the WHOLE slice (a group may hold no fit at all): no failure, and at least a third of the fitted instances
    compared record by record - the ratio of tests/test_gpu_frames.py::test_randomised_sweep.  A reported eigen-gap below 1e-9 takes a
    record out of the comparison only where the oracle's own gap is small too (FM.check_run), so a library that reported no gap
    would fail here, not pass unchecked."""
    fails = []
    tally = FM.new_tally()
    for s in S.FORMAT_SEEDS:
        c = FM.make_case(s)
        for r in FM.RUNS:
            if r["entry"] == "fit" and FM.applies(c, r):
                try:
                    got = FM.run_gpu(c, r)
                except Exception as e:   # noqa: BLE001
                    pytest.fail(_report(fails + [f"seed {s} {r}: call failed, nothing more was run: {e!r}"]))
                FM.tally_call(tally, r)
                fails += [f"seed {s} {r}: {m}" for m in FM.check_run(c, FM.oracle_case(s), r, got, rules=("fit",), tally=tally)]
    print("\n".join(FM.tally_lines(tally)))
    assert not fails, _report(fails)
    assert tally["fitted"] > 0 and 3 * tally["compared"] >= tally["fitted"], (tally["compared"], tally["fitted"])


@pytest.mark.parametrize("seeds", _groups(S.ALIGN_RANSAC_SEEDS, 6), ids=lambda v: str(v[0]))
def test_align_ransac_campaign_slice(gpu, seeds):
    """ransac_scale_batch / ransac_subsets / align_depth_batch against the NumPy restatement (tests/align_ransac_cases.py): status,
    n_trials, n_inliers and best_trial exactly and coef to the adjacent float32 on every decided frame, one of the oracle's own walks
    on an undecided one (classes from the oracle alone), the runs among each other bit for bit, every drawn row, every pixel of the
    aligned maps.  A call that raises ends the group's GPU work."""
    fails = []
    tally = AR.new_tally()
    for s in seeds:
        c = AR.make_case(s)
        want = AR.oracle_case(s)
        AR.tally_case(tally, c, want)
        cache, default = {}, None
        for r in AR.RUNS:
            if not AR.applies(c, r):
                continue
            try:
                got = AR.run_gpu(c, r, cache)
            except Exception as e:   # noqa: BLE001 - whatever made the call fail is looked at before anything else runs on the device
                print("\n".join(AR.tally_lines(tally)))
                pytest.fail(_report(fails + [f"seed {s} {r}: call failed, nothing more was run: {e!r}"]))
            tally["calls"] += 1
            if not r:
                default = got
            fails += [f"seed {s} {r}: {m}" for m in AR.check_run(c, want, r, got, default, tally)]
    print("\n".join(AR.tally_lines(tally)))
    assert not fails, _report(fails)


def test_engine_slice_reaches_the_documented_refusal(gpu):
    """The slice's frame above 1 Mpx is refused loudly in annotation mode (include/la3d.h) - and fitted in full through the u8 entry."""
    s = next(s for s in S.ENGINE_SEEDS if np.prod(E.make_case(s)["masks"].shape[1:]) > 1 << 20)
    c = E.make_case(s)
    with pytest.raises(Exception, match="bit image in LDS") as e:
        E.run_gpu(c, dict(entry="rle"))
    assert E.documented_refusal(c, dict(entry="rle"), e.value)
    if c["sidx"] is None:
        assert not E.check_run(c, E.oracle_case(s)[1:], {}, E.run_gpu(c, {}))
