"""CPU-only contract of the argument checks of the bit-plane entries (labelany3d_amd/csrc/la3d_bits.hip, la3d_rle_encode.hip,
la3d_open.hip; one check routine for the packers, in la3d_bitplanes.hpp): every refusal keeps its return code, its message byte for
byte, and its rank among the other refusals of its entry.  The expectations (tests/golden/packer_refusals.json) were recorded with
tests/packer_refusal_cases.py from the library of the commit BEFORE the checks were folded into one routine - and, for the crop
packers, the run-length encoder and the opening, of the commit before their code moved to units of its own; they are data, never
regenerated from the tree under test."""
import json
import os

from . import packer_refusal_cases as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packer_refusals.json")
PACKERS = ("la3d_pack_mask_bits", "la3d_pack_logits_bits", "la3d_unpack_mask_bits", "la3d_mask_stats_bits", "la3d_pack_rle_bits",
           "la3d_pack_poly_bits", "la3d_pack_rle_bits_frames", "la3d_pack_poly_bits_frames", "la3d_pack_label_bits",
           "la3d_pack_label_bits_frames", "la3d_pack_mask_bits_frames", "la3d_pack_logits_bits_frames", "la3d_pack_crop_bits",
           "la3d_pack_crop_bits_frames", "la3d_open_bits", "la3d_open_bits_frames")
BLOCKS = ("la3d_rle_encode_offsets", "la3d_rle_encode")    # one argument: a la3d_rle_encode_args block
ERR_ARG, ERR_UNSUPPORTED = -1, -2          # (LA3D_ERR_HIP = -3 would mean that a case reached a launch)


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
        by.setdefault(entry, []).append((case, rc, msg))
        assert rc in (0, ERR_ARG, ERR_UNSUPPORTED), (entry, case, rc)          # refused or nothing to do: no case reached a launch
        assert (rc == 0) == (msg == "") and (rc == 0 or msg.startswith(entry + ": ")), (entry, case, msg)
    assert set(PACKERS + BLOCKS) <= set(by) and len(by) == len(PACKERS) + len(BLOCKS) + 2   # (+ la3d_rle_decode / la3d_poly_decode)
    for entry in PACKERS:
        cases = {c: (rc, msg) for c, rc, msg in by[entry]}
        assert cases["B=-1"][0] == cases["H=0"][0] == cases["W=0"][0] == ERR_ARG, entry
        assert cases["B=0"][0] == 0, entry
        assert any(c.endswith("=NULL") and rc == ERR_ARG for c, (rc, _) in cases.items()), entry
        assert any(c.endswith("misaligned") and rc == ERR_ARG for c, (rc, _) in cases.items()), entry
    for entry in BLOCKS:
        cases = {c: (rc, msg) for c, rc, msg in by[entry]}
        assert cases["B=-1"][0] == cases["H=0"][0] == cases["W=0"][0] == ERR_ARG, entry
        assert any(c.endswith("=NULL") and rc == ERR_ARG for c, (rc, _) in cases.items()), entry
        assert any(c.endswith("misaligned") and rc == ERR_ARG for c, (rc, _) in cases.items()), entry
    # (the first stage writes offsets[0] on the stream for B = 0 too: that call is a launch, so only the second stage has the case)
    assert {c: rc for c, rc, _ in by["la3d_rle_encode"]}["B=0"] == 0 and "B=0" not in {c for c, _, _ in by["la3d_rle_encode_offsets"]}
    # the pairs whose precedence the older contract tests pin
    for entry in ("la3d_pack_mask_bits", "la3d_pack_label_bits", "la3d_pack_label_bits_frames", "la3d_pack_mask_bits_frames"):
        rc, msg = {c: (rc, msg) for c, rc, msg in by[entry]}["too large before B=0"]
        assert rc == ERR_ARG and "too large" in msg, entry
    for entry in ("la3d_pack_rle_bits", "la3d_pack_poly_bits", "la3d_pack_crop_bits") + BLOCKS:
        rc, msg = {c: (rc, msg) for c, rc, msg in by[entry]}["LDS bound before short stride"]
        assert rc == ERR_UNSUPPORTED and "must fit LDS" in msg, entry
    # the source rules of the crop packers rank in front of the packers' own; the opening's overlap rule and its B = 0
    for entry in ("la3d_pack_crop_bits", "la3d_pack_crop_bits_frames"):
        cases = {c: (rc, msg) for c, rc, msg in by[entry]}
        assert all(cases[c][0] == ERR_ARG and "bad source" in cases[c][1] for c in ("source before sizes", "source before B=0", "source before LDS bound")), entry
        assert "place" in cases["place before NULL"][1], entry
    for entry in ("la3d_open_bits", "la3d_open_bits_frames"):
        cases = {c: (rc, msg) for c, rc, msg in by[entry]}
        assert cases["in place"][0] == ERR_ARG and "overlap" in cases["in place"][1], entry
        assert cases["k before B=0"][0] == ERR_ARG and cases["too many bands"][0] == ERR_UNSUPPORTED, entry
