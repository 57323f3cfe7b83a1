"""Writes tests/golden/g20_components.npz: what ``scipy.ndimage.label`` itself gives on the fixture planes of tests/components_cases.py,
for both connectivities and the three rules (all, min_area, largest).  Small frames store the packed output plane, the statistics and
the first TABLE_ROWS table rows; the three 480 x 640 planes store the statistics, the table rows and a SHA-256 of the output words
(stored 640 wide).  Only data is written; needs SciPy.  The committed fixture was written with python 3.10.12, numpy 2.2.6, scipy 1.15.3
(the fixture's ``scipy`` entry holds the last).

    python tests/golden/make_golden_components.py
"""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import components_cases as CC  # noqa: E402

STRUCTURE = {4: ndimage.generate_binary_structure(2, 1), 8: np.ones((3, 3), int)}


def scipy_components(mask, conn, min_area, largest):
    labels, n = ndimage.label(mask, STRUCTURE[conn])
    areas = np.bincount(labels.reshape(-1), minlength=n + 1)[1:]
    table = np.zeros((n, 5), np.int32)
    for j, sl in enumerate(ndimage.find_objects(labels)):
        table[j] = [areas[j], sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start]
    kept = np.flatnonzero(areas >= min_area)
    if largest and len(kept):
        best = areas[kept].max()
        kept = kept[areas[kept] == best][:1]
    out = np.isin(labels, kept + 1)
    stats = np.asarray([n, len(kept), int(mask.sum()), int(out.sum()), *CC.rect(out)], np.int32)
    tab = np.zeros((CC.TABLE_ROWS, 5), np.int32)
    tab[:min(n, CC.TABLE_ROWS)] = table[:CC.TABLE_ROWS]
    return out, stats, tab


def main():
    small, big = CC.fixture_planes(), CC.big_planes()
    data = {"frames": np.asarray(CC.FIXTURE_FRAMES, np.int32), "big_frame": np.asarray(CC.BIG_FRAME, np.int32),
            "scipy": np.asarray(scipy.__version__), "big_runs": np.asarray([CC.count_runs(m) for m in big], np.int32)}
    for f, planes in enumerate(small):
        data[f"in_{f}"] = CC.pack(planes)
    for key, f, p, conn, min_area, largest in CC.fixture_keys():
        mask = big[p] if f < 0 else small[f][p]
        out, stats, tab = scipy_components(mask, conn, min_area, largest)
        data[f"stats_{key}"], data[f"table_{key}"] = stats, tab
        if f < 0:
            data[f"sha_{key}"] = np.frombuffer(bytes.fromhex(CC.words_sha256(out, CC.BIG_FRAME[1])), np.uint8)
        else:
            data[f"out_{key}"] = CC.pack(out[None])[0]
    np.savez_compressed(CC.GOLDEN, **data)
    print(CC.GOLDEN, "runs of the big planes:", data["big_runs"].tolist(),
          "components (8):", [int(data[f"stats_big_{p}_8_0"][0]) for p in range(len(big))])


if __name__ == "__main__":
    main()
