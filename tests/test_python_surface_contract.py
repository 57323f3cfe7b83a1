"""CPU-only: the Python surface of the package against its recording (tests/golden/python_surface.json, made by
tests/golden/make_python_surface.py at the commit before the Python layer was put in one-way order).  Modules may be split and merged;
what a caller can name, how it is called and what its docstring promises may not change along the way.  Source hashes are recorded
too but not asserted: ``make_python_surface.py --report`` lists the bodies that changed."""
import functools
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

RETIRED = {"_open_frames_check": "two lines now: _tabled (frames.py) and _open_scalars (morph.py), at its two call sites"}
"""The only recorded name that may be absent.  The other duplicates that were merged had no name of their own: the three copies of the
"frames must be a PackedFrames / ... / FrameGrid" test and the inline flat-``out`` test are ``frames._tabled`` / ``frames._flat_out``."""


def _maker():
    spec = importlib.util.spec_from_file_location("_make_python_surface", os.path.join(HERE, "golden", "make_python_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _both():
    """(the recording, the surface of this tree, the maker) - computed once for the module, read only"""
    mk = _maker()
    with open(mk.PATH) as fh:
        return json.load(fh), mk.surface(), mk


def test_the_recording_is_what_the_issue_counted():
    pinned, _, _ = _both()
    assert len(pinned["objects"]) == 297 and len(pinned["public"]) == 123
    assert all(set(v) == {"module", "signature", "doc", "source"} for v in pinned["objects"].values())
    assert "0x" not in json.dumps(pinned) and os.sep + "root" not in json.dumps(pinned)     # nothing of one process or one checkout


def test_every_public_name_of_the_package_is_still_there():
    import labelany3d_amd as la

    pinned, now, _ = _both()
    assert [n for n in pinned["public"] if not hasattr(la, n)] == []
    assert [n for n in pinned["public"] if n not in now["public"]] == []
    assert sorted(set(la.__all__) - set(now["public"])) == []


def test_every_recorded_object_keeps_its_signature_and_docstring():
    pinned, now, mk = _both()
    absent = [n for n in pinned["objects"] if n not in now["objects"]]
    assert sorted(absent) == sorted(RETIRED), "the recorded names that no module defines any more are exactly the retired ones"
    rep = mk.report(pinned, now)
    assert rep["changed_signature"] == []
    assert rep["changed_doc"] == []
    assert rep["public_lost"] == []
    # (moved homes and changed bodies are what a refactor does: reported by ``--report``, not judged here)
    assert set(rep) == {"moved", "changed_source", "changed_signature", "changed_doc", "absent", "new", "public_lost"}
