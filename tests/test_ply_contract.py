"""CPU-only: ``labelany3d_amd.ply.write_ply`` round-trips through a small reader written here (the format is the documented one:
binary little-endian, three float properties), an empty cloud included; the export options of the scene pipeline exist and are off
by default."""
import inspect

import numpy as np
import pytest


def read_ply(path):
    """the documented subset: binary_little_endian 1.0, one vertex element of three float properties x, y, z -> (N, 3) float32"""
    with open(path, "rb") as f:
        data = f.read()
    head, sep, body = data.partition(b"end_header\n")
    assert sep, "no end_header"
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    n, props = None, []
    for ln in lines[2:]:
        tok = ln.split()
        if tok[:2] == ["element", "vertex"]:
            n = int(tok[2])
        elif tok[:1] == ["element"]:
            raise AssertionError(f"unexpected element: {ln}")
        elif tok[:1] == ["property"]:
            props.append(tuple(tok[1:]))
    assert props == [("float", "x"), ("float", "y"), ("float", "z")], props
    assert n is not None and len(body) == 12 * n, (n, len(body))
    return np.frombuffer(body, "<f4").reshape(n, 3)


@pytest.mark.parametrize("n", [0, 1, 7, 1000])
def test_write_ply_round_trips(tmp_path, n):
    from labelany3d_amd.ply import write_ply

    rs = np.random.RandomState(n)
    pts = rs.uniform(-5, 5, (n, 3))
    path = tmp_path / "cloud.ply"
    write_ply(str(path), pts)
    got = read_ply(str(path))
    assert got.dtype == np.float32 and got.shape == (n, 3)
    np.testing.assert_array_equal(got, pts.astype(np.float32))
    write_ply(str(path), pts.astype(np.float32)[::-1])                  # a float32 view that is not contiguous
    np.testing.assert_array_equal(read_ply(str(path)), pts.astype(np.float32)[::-1])


def test_write_ply_refuses_other_shapes(tmp_path):
    from labelany3d_amd.ply import write_ply

    for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError, match=r"\(N, 3\)"):
            write_ply(str(tmp_path / "bad.ply"), bad)


def test_the_export_is_an_option_that_is_off_by_default():
    from labelany3d_amd import fit_scenes

    sig = inspect.signature(fit_scenes.ScenePipeline.__init__).parameters
    assert sig["export_points"].default is False and sig["points_dir"].default == "points"
    args = fit_scenes.build_parser().parse_args(["--scenes", "x"])
    assert args.export_points is False and args.points_dir == "points"
    args = fit_scenes.build_parser().parse_args(["--scenes", "x", "--export-points", "--points-dir", "clouds"])
    assert args.export_points is True and args.points_dir == "clouds"
