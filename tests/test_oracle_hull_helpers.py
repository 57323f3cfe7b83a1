"""CPU pins of the oracle helpers the convex-hull campaign rests on (oracle/la3d_oracle.py): the edge table against the walk of
yaw_convex_hull, the pre-sorted monotone chain against the one yaw_convex_hull uses, the yaw override of estimate_bbox."""
import numpy as np
import pytest

from oracle import la3d_oracle as O


def clouds(seed, count):
    """Footprints where a chain can go wrong: Gaussian blobs, integer grids (collinear runs, duplicates), points drawn with
    replacement (the reference's subsample), rays through the origin (the column structure of a depth map), collinear sets, 0 - 3
    points."""
    rs = np.random.RandomState(seed)
    for k in range(count):
        kind = k % 6
        n = int(rs.choice([0, 1, 2, 3, 4, 7, 20, 64, 300]))
        if kind == 0:
            xz = rs.randn(n, 2) * rs.uniform(0.1, 5, 2) + rs.uniform(-3, 3, 2)
        elif kind == 1:
            xz = rs.randint(-4, 5, (n, 2)).astype(float)
        elif kind == 2:
            base = rs.randn(max(n // 3, 1), 2)
            xz = base[rs.randint(0, len(base), n)]
        elif kind == 3:
            slope = rs.uniform(-1, 1, max(n // 2, 1))
            d = rs.choice([1.0, 2.5, -1.0, 0.0, 4.0], (n,))
            xz = np.stack([d * slope[rs.randint(0, len(slope), n)], d], 1)
        elif kind == 4:
            t = rs.randint(-5, 6, n).astype(float)
            xz = np.stack([t * 0.5, t * 0.25 + 1.0], 1)
        else:
            xz = np.round(rs.randn(n, 2), 1)
        pc = np.zeros((n, 3))
        pc[:, 0], pc[:, 2], pc[:, 1] = xz[:, 0], xz[:, 1], rs.randn(n)
        yield pc


def test_presorted_chain_is_the_chain():
    n = 0
    for pc in clouds(20261017, 360):
        pts = pc[:, [0, 2]]
        assert O._monotone_chain_presorted(pts) == O._monotone_chain(pts)
        n += 1
    assert n == 360


def test_yaw_convex_hull_is_the_first_strict_minimum_of_the_edge_table():
    tables = fallbacks = 0
    for pc in clouds(7, 360):
        table = O.hull_edge_table(pc)
        if len(pc) == 0:
            assert table is None
            continue
        hull = O._monotone_chain(pc[:, [0, 2]])
        if table is None:
            assert len(hull) < 3
            fallbacks += 1
            continue
        yaws, areas = table
        assert len(yaws) == len(areas) == len(hull) >= 3
        assert O.yaw_convex_hull(pc) == yaws[int(np.argmin(areas))]   # (argmin: the first of equal minima = the first STRICT minimum)
        tables += 1
    assert tables >= 100 and fallbacks >= 50
    pc = np.array([[0.0, 0, 1], [1, 0, 1], [np.inf, 0, 2], [0, 0, 2]])
    assert O.hull_edge_table(pc) is None   # a non-finite coordinate: yaw_convex_hull hands over to PCA (which raises)


def test_yaw_override_gives_the_box_under_that_yaw():
    rs = np.random.RandomState(3)
    pts = rs.randn(200, 3) * [2.0, 0.3, 0.7] + [0.5, 1.0, 6.0]
    g = np.array([0.05, -0.97, 0.1, 1.2])
    for ground in (None, g):
        v, c, d, R, a = O.estimate_bbox(pts, None, ground, "convex_hull", rand_ind=False, return_aux=True)
        v2, c2, d2, R2, a2 = O.estimate_bbox(pts, None, ground, "convex_hull", rand_ind=False, return_aux=True, yaw=a["yaw"])
        for x, y in ((v, v2), (c, c2), (d, d2), (R, R2)):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
        # a quarter turn: the same rectangle, length and width exchanged, the same centre
        v3, c3, d3, R3 = O.estimate_bbox(pts, None, ground, "pca", rand_ind=False, yaw=a["yaw"] + np.pi / 2)
        np.testing.assert_allclose(c3, c, atol=1e-12)
        np.testing.assert_allclose(d3, [d[2], d[1], d[0]], atol=1e-12)
        rec = O.fit_points(pts, ground, False, "convex_hull", yaw=0.25)[0]
        assert np.isfinite(rec).all() and not np.allclose(rec[6:15], np.ravel(R))
    with pytest.raises(ValueError, match="No valid points"):
        O.estimate_bbox(np.full((3, 3), np.nan), None, None, "convex_hull", rand_ind=False, yaw=0.1)
