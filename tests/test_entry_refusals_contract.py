"""CPU-only contract of the argument checks of the C entries outside the bit-plane units (labelany3d_amd/csrc/la3d.hip - the fit
entries and fit_dispatch -, la3d_instance.hip, la3d_points.hip, la3d_masks.hip, la3d_consumers.hip, la3d_depth16.hip, la3d_align.hip;
one refusal helper for all of them, refuse() in la3d_device.hpp): every refusal keeps its return code, its message byte for byte,
and its rank among the other refusals of its entry.  The expectations (tests/golden/entry_refusals.json) were recorded with
tests/entry_refusal_cases.py from the library of commit 3267327, the commit BEFORE the checks were rewritten onto that helper and the
fit entries came to share their block copy; they are data, never regenerated from the tree under test."""
import json
import os

from . import entry_refusal_cases as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entry_refusals.json")
ERR_ARG, ERR_UNSUPPORTED = -1, -2          # (LA3D_ERR_HIP = -3 would mean that a case reached a launch)
FIT = ("la3d_fit_instances", "la3d_fit_instances_rle", "la3d_fit_instances_poly", "la3d_fit_instances_rle_filtered",
       "la3d_fit_instances_poly_filtered", "la3d_fit_instances_ex", "la3d_fit_instances_bits", "la3d_fit_instances_depth16",
       "la3d_fit_instances_frames", "la3d_fit_instances_frames_depth16", "la3d_fit_instances_frames_bits")
BLOCKS = FIT[5:] + ("la3d_fit_annotations_host",)    # a la3d_fit_args block: the first-published size is the smallest they take
OTHERS = ("la3d_fit_points", "la3d_estimate_bbox_host", "la3d_unproject_host", "la3d_fit_annotations_host", "la3d_unproject",
          "la3d_unproject_batch", "la3d_pad_rows", "la3d_mask_counts", "la3d_mask_stats_poly", "la3d_mask_stats", "la3d_mask_stats_rle",
          "la3d_masked_ratio_median", "la3d_align_select_batch", "la3d_align_select", "la3d_align_apply", "la3d_unproject_matches",
          "la3d_project_boxes", "la3d_iou_matrix", "la3d_pack_depth16", "la3d_unpack_depth16", "la3d_align_ransac_batch",
          "la3d_align_ransac_subsets", "la3d_align_apply_batch")


def _want():
    return json.load(open(GOLDEN))["cases"]


def test_every_refusal_is_the_recorded_one():
    from labelany3d_amd import _lib

    got, want = RC.run(_lib.lib), _want()
    assert [g[:2] for g in got] == [w[:2] for w in want]                     # the same cases, in the same order
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, wrong[:5]


def test_the_fixture_covers_every_entry_and_every_kind_of_refusal():
    want = _want()
    by = {}
    for entry, case, rc, msg in want:
        by.setdefault(entry, {})[case] = (rc, msg)
        assert rc in (0, ERR_ARG, ERR_UNSUPPORTED), (entry, case, rc)          # refused or nothing to do: no case reached a launch
        assert (rc == 0) == (msg == "") and (rc == 0 or msg.startswith(entry + ": ")), (entry, case, msg)
    assert set(by) == set(FIT + OTHERS)
    for entry in FIT:
        c = by[entry]
        assert c["B=-1"] == c["H=0"] == c["W=0"] == c["K=NULL"] == (ERR_ARG, entry + ": bad argument"), entry
        assert c["B=0"][0] == 0 and c["B=0 before workspace"][0] == 0, entry
        assert c["H*W > 2^28 before B=0"][0] == ERR_ARG and "workspace" in c["workspace=NULL"][1] and "workspace" in c["workspace misaligned"][1], entry
    for entry in BLOCKS:
        c = by[entry]
        assert c["args=NULL"] == c["struct_size=0"] == c[f"struct_size={RC.V1 - 1}"] == (ERR_ARG, entry + ": bad struct_size"), entry
        assert c["a longer block is read"][0] == ERR_ARG and "struct_size" not in c["a longer block is read"][1], entry
    # the pairs whose precedence the older contract tests pin: workspace first, filter before the LDS bound
    for entry in FIT[1:]:
        rc, msg = by[entry]["workspace before LDS bound"]
        assert rc == ERR_ARG and "workspace" in msg and by[entry]["LDS bound"][0] == ERR_UNSUPPORTED, entry
    for entry in ("la3d_fit_instances_rle_filtered", "la3d_fit_instances_poly_filtered"):
        assert "fused filter" in by[entry]["filter before LDS bound"][1] and "workspace" in by[entry]["workspace before filter"][1], entry
    # behind fit_dispatch: each of the three instance units refuses by itself, the frames entries name the tiled form
    sub = "reference-subsample mode needs the bit image in LDS"
    assert sub in by["la3d_fit_instances_ex"]["subsample mode without the bit image in LDS"][1]
    assert all(sub in by["la3d_fit_instances_depth16"][f"{t}: subsample mode without the bit image in LDS"][1] for t in ("F16", "U16"))
    for entry, tag in (("la3d_fit_instances_frames", ""), ("la3d_fit_instances_frames_depth16", "F16: "), ("la3d_fit_instances_frames_depth16", "U16: "),
                       ("la3d_fit_instances_frames_bits", ""), ("la3d_fit_instances_frames_bits", "F16: "), ("la3d_fit_instances_frames_bits", "U16: ")):
        rc, msg = by[entry][tag + "bounds outside the tiled form"]
        assert rc == ERR_UNSUPPORTED and msg.startswith(entry + ": bounds outside the tiled form"), (entry, tag)
        rc, msg = by[entry][tag + "subsample mode: bounds outside the tiled form"]
        assert rc == ERR_UNSUPPORTED and msg.startswith(entry + ": reference-subsample mode: bounds outside the tiled form"), (entry, tag)
    # the other units: every entry is refused at least once, and an entry with a "nothing to do" case ranks its first rule in front of it
    for entry in OTHERS:
        assert any(rc == ERR_ARG for rc, _ in by[entry].values()), entry
    for entry, first, nothing in (("la3d_fit_points", "method before B=0", "B=0"), ("la3d_unproject_batch", "bad argument before P=0", "P=0"),
                                  ("la3d_mask_stats_poly", "H*W > 2^20 before B=0", "B=0"), ("la3d_pack_depth16", "sizes before P=0", "P=0"),
                                  ("la3d_unpack_depth16", "sizes before P=0", "P=0"), ("la3d_align_ransac_batch", "too many trials before P=0", "P=0"),
                                  ("la3d_align_ransac_subsets", "too many trials before P=0", "P=0"), ("la3d_fit_annotations_host", "bad argument before B=0", "B=0")):
        assert by[entry][first][0] < 0 and by[entry][nothing][0] == 0, entry
    # ... and the LDS bounds that come behind "nothing to do"
    for entry, bound, nothing in (("la3d_mask_stats_poly", "too many rows for LDS", "B=0 before too many rows"),
                                  ("la3d_masked_ratio_median", "frame too large for LDS", "B=0 before too large"),
                                  ("la3d_align_apply_batch", "frame too large", "P=0 before too large")):
        assert by[entry][bound][0] == ERR_UNSUPPORTED and by[entry][nothing][0] == 0, entry
