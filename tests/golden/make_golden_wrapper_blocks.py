"""Writes tests/golden/wrapper_blocks.json: what every case of tests/test_gpu_wrapper_blocks.py sends to the library (entry, argument
block, call count, returned shapes), recorded on a GPU with the Python layer whose behaviour is to be pinned - the commit BEFORE the
wrappers were rebuilt on one call builder (a worktree of that commit with this file and the test module copied in):

    python tests/golden/make_golden_wrapper_blocks.py [output path]

The file is data only.  Cases whose wrapper raised are listed on stderr: the test accepts none."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.test_gpu_wrapper_blocks import CASES, ENTRIES, FIXTURE, record  # noqa: E402


def main(path=FIXTURE):
    from labelany3d_amd import _lib

    real = {e: getattr(_lib.lib, e) for e in ENTRIES}
    out = {}
    for name in CASES:
        out[name] = record(name, setattr)
        for e, f in real.items():
            setattr(_lib.lib, e, f)
        if "raises" in out[name]:
            print(f"{name}: {out[name]['raises']}", file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases, {sum(len(v['calls']) for v in out.values())} C calls -> {path}")


if __name__ == "__main__":
    main(*sys.argv[1:2])
