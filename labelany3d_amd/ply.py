"""Point clouds as PLY files: what ``ScenePipeline(export_points=True)`` writes per fitted object.

The format is the smallest binary PLY: ``format binary_little_endian 1.0``, ``element vertex N`` and three ``property float``
fields x, y, z, then N * 12 bytes of little-endian float32.  The reference writes its clouds through trimesh; byte parity with
trimesh's writer (its comment line, its property order for coloured clouds) is NOT claimed - any PLY reader takes both."""
from __future__ import annotations

import numpy as np

_HEADER = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n"


def write_ply(path, points) -> None:
    """``points`` (N, 3), any float dtype (N may be 0) -> a binary little-endian PLY of float32 vertices at ``path``."""
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be (N, 3), got {pts.shape}")
    pts = np.ascontiguousarray(pts, dtype="<f4")
    with open(path, "wb") as f:
        f.write((_HEADER % len(pts)).encode("ascii"))
        f.write(pts.tobytes())
