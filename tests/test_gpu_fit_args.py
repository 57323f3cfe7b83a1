"""GPU tests of the one argument block every fit call goes through: the five legacy C entries (which no Python wrapper calls any
more) give exactly what la3d_fit_instances_ex gives for the equivalent block, and the wrappers over _ex check their inputs."""
import ctypes as C

import numpy as np
import pytest

from oracle import la3d_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def _batch(seed=5, B=12, H=96, W=128):
    rs = np.random.RandomState(seed)
    depth = rs.uniform(0.5, 10, (B, H, W)).astype(np.float32)
    masks = np.zeros((B, H, W), bool)
    segs = []
    for i in range(B - 1):    # the last instance stays empty
        h, w = rs.randint(6, H - 10), rs.randint(6, W - 10)
        r0, c0 = rs.randint(0, H - h), rs.randint(0, W - w)
        masks[i, r0:r0 + h, c0:c0 + w] = True
        segs.append([[c0, r0, c0 + w - 1, r0, c0 + w - 1, r0 + h - 1, c0, r0 + h - 1]])
    segs.append([])
    K = np.array([[150.0, 0, 64], [0, 150.0, 48], [0, 0, 1]])
    ground = np.array([[0.02, -0.98, 0.1, 1.5]] * B) + 0.03 * rs.randn(B, 4)
    return depth, masks, segs, K, ground


@pytest.mark.parametrize("grounded", [False, True])
@pytest.mark.parametrize("kind", ["u8", "rle", "poly", "rle_filtered", "poly_filtered"])
def test_legacy_entries_equal_ex(la, kind, grounded):
    import torch

    from labelany3d_amd._lib import FitArgs, lib

    depth, masks, segs, K, ground = _batch()
    B, H, W = masks.shape
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), device=dev).to(dt)   # noqa: E731
    d, k = t(depth, torch.float32), t(K[None], torch.float64)
    g = t(ground, torch.float64) if grounded else None
    m = t(masks.view(np.uint8), torch.uint8)
    c, o, _, _ = la.pack_rle([O.rle_encode(x) for x in masks])
    c, o = t(c, torch.int32), t(o, torch.int64)
    xy, ro, ir, _, _ = la.pack_polygons(segs, H, W)
    xy, ro, ir = t(xy, torch.int32), t(ro, torch.int64), t(ir, torch.int64)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())   # noqa: E731
    res = []
    for use_ex in (False, True):
        f = la.InstanceFitter(B, H, W, dev)
        f.boxes.fill_(-1.0); f.aux.fill_(-1.0); f.status.fill_(-1)
        stats = torch.full((B, 4), -1, dtype=torch.int32, device=dev)
        head = [p(d), H * W, None]
        cam = [p(k), 0, p(g), None, B, H, W]
        outs = [p(f.boxes[0]), p(f.status[0]), p(f.aux[0])]
        tail = [p(f.workspace[0]), C.c_void_p(torch.cuda.current_stream().cuda_stream)]
        filt = [10, 100, 10]
        if use_ex:
            a = FitArgs(struct_size=C.sizeof(FitArgs), B=B, H=H, W=W, depth=p(d), depth_plane_stride=H * W, K=p(k), ground=p(g),
                        out=outs[0], status=outs[1], aux=outs[2], workspace=tail[0], stream=tail[1])
            if kind == "u8":
                a.mask = p(m)
            elif kind.startswith("rle"):
                a.rle_counts, a.rle_offsets = p(c), p(o)
            else:
                a.poly_xy, a.ring_offsets, a.inst_rings = p(xy), p(ro), p(ir)
            if kind.endswith("_filtered"):
                a.filter_boundary, a.filter_min_area, a.filter_max_edge = filt
                a.stats = p(stats)
            rc = lib.la3d_fit_instances_ex(C.byref(a))
        elif kind == "u8":
            rc = lib.la3d_fit_instances(*head, p(m), *cam, *outs, *tail)
        else:
            src = [p(c), p(o)] if kind.startswith("rle") else [p(xy), p(ro), p(ir)]
            name = "la3d_fit_instances_" + kind
            extra = ([*filt] if kind.endswith("_filtered") else [])
            post = outs + ([p(stats)] if kind.endswith("_filtered") else []) + tail
            rc = getattr(lib, name)(*head, *src, *cam, *extra, *post)
        assert rc == 0, lib.la3d_last_error().decode()
        torch.cuda.synchronize()
        res.append([x.cpu().numpy().copy() for x in (f.boxes[0], f.status[0], f.aux[0], stats)])
    (b0, s0, a0, t0), (b1, s1, a1, t1) = res
    assert (s0 == 0).any() and (s0 != 0).any()                     # a real batch: boxes fitted, the empty mask rejected
    np.testing.assert_array_equal(s0, s1)
    assert b0.tobytes() == b1.tobytes() and a0.tobytes() == a1.tobytes()   # bit for bit (NaN records included)
    np.testing.assert_array_equal(t0, t1)
    if kind.endswith("_filtered"):
        assert (t0[:, 0] >= 0).all()


@pytest.mark.parametrize("kind", ["rle", "poly", "ex"])
def test_wrappers_reject_bad_inputs(la, kind):
    depth, masks, segs, K, ground = _batch(B=4)
    B, H, W = masks.shape
    rles = [O.rle_encode(x) for x in masks]

    def call(K=K, **kw):
        if kind == "rle":
            return la.fit_instances_rle(depth, rles, K, **kw)
        if kind == "poly":
            return la.fit_instances_poly(depth, la.pack_polygons(segs, H, W), K, **kw)
        return la.fit_instances_ex(depth, K, rles=rles, **kw)

    call(ground=ground, image_index=np.arange(B, dtype=np.int32))     # (the well-formed call runs)
    with pytest.raises(ValueError, match="ground must be"):
        call(ground=ground[:, :3])
    with pytest.raises(ValueError, match="sample_idx must be"):
        call(sample_idx=np.zeros((B, 499), np.int32))
    with pytest.raises(ValueError, match="out of range"):
        call(image_index=np.full(B, B, np.int32))
    with pytest.raises(ValueError, match="out of range"):
        call(image_index=np.full(B, -1, np.int32), ground=ground)
    with pytest.raises(ValueError, match=r"image_index must be \(B,\)"):
        call(image_index=np.zeros(B + 1, np.int32))
    with pytest.raises(ValueError, match="K must be"):
        call(K=np.eye(4))
