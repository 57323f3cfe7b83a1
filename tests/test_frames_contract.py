"""CPU-only contract of the frames call (include/la3d.h "images of different sizes in one call"): the exports exist on every layer,
``la3d_frame`` has the layout the header states, ``pack_frames`` lays the planes out as documented, the argument errors come
before any device work, and ``ScenePipeline(mixed_frames=True)`` batches images of different sizes in arrival order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    assert re.search(r"\bla3d_fit_instances_frames\s*\(", hdr)
    assert "la3d_fit_instances_frames" in _lib.EXPORTS and hasattr(_lib.lib, "la3d_fit_instances_frames")
    for fn in ("pack_frames", "fit_instances_frames", "PackedFrames"):
        assert callable(getattr(la, fn)) and fn in la.__all__
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2   # additive: the ABI version stays


def test_frame_row_layout_is_the_headers():
    """sizeof(la3d_frame) == 24 and the field offsets of the header's struct, on the ctypes struct and on the NumPy dtype of the table"""
    from labelany3d_amd import _lib, masks

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    body = re.search(r"typedef struct la3d_frame \{(.*?)\} la3d_frame;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == [("depth_offset", "int64_t"), ("H", "int32_t"), ("W", "int32_t"), ("frame_width", "int32_t"), ("reserved", "int32_t")]
    size = {"int64_t": 8, "int32_t": 4}
    off, want = 0, {}
    for name, ctype in fields:
        want[name] = off
        off += size[ctype]
    assert off == 24
    assert C.sizeof(_lib.Frame) == 24 and masks.FRAME_DTYPE.itemsize == 24
    assert [n for n, _ in _lib.Frame._fields_] == [n for n, _ in fields] == list(masks.FRAME_DTYPE.names)
    for name, _ in fields:
        assert getattr(_lib.Frame, name).offset == want[name] == masks.FRAME_DTYPE.fields[name][1]
        assert getattr(_lib.Frame, name).size == masks.FRAME_DTYPE.fields[name][0].itemsize
    # the argument block did not change
    assert C.sizeof(_lib.FitArgs) == 232 and _lib.FitArgs.method.offset == 224


def test_pack_frames_layout():
    import torch

    from labelany3d_amd import pack_frames, padded_width
    from labelany3d_amd.masks import FRAME_DTYPE

    rs = np.random.RandomState(3)
    sizes = [(480, 640), (640, 480), (427, 640), (375, 500), (500, 333), (96, 224), (5, 7), (8, 32), (33, 65)]
    maps = [rs.uniform(0.5, 9, s).astype(np.float32) for s in sizes]
    maps[3] = torch.as_tensor(maps[3])                       # tensors and arrays mix
    pf = pack_frames(maps, device="cpu")
    assert pf.sizes == sizes and pf.table_host.dtype == FRAME_DTYPE and len(pf.table_host) == len(sizes)
    assert pf.H == 640 and pf.W == 640
    assert pf.depth.dtype == torch.float32 and pf.depth.dim() == 1
    assert pf.table.dtype == torch.int32 and tuple(pf.table.shape) == (len(sizes), 6)
    np.testing.assert_array_equal(pf.table.numpy().view(np.uint8).reshape(-1), pf.table_host.view(np.uint8).reshape(-1))
    flat = pf.depth.numpy()
    covered = np.zeros(flat.shape, bool)
    end = 0
    for p, ((h, w), row) in enumerate(zip(sizes, pf.table_host)):
        off, H, Wp, fw, res = (int(row[k]) for k in FRAME_DTYPE.names)
        assert (H, Wp, fw, res) == (h, padded_width(w), w, 0)
        assert Wp % 32 == 0 and off % 4 == 0 and off >= end          # pitch of whole words, 16-byte aligned, no overlap
        plane = flat[off:off + H * Wp].reshape(H, Wp)
        np.testing.assert_array_equal(plane[:, :w], np.asarray(maps[p]))
        assert (plane[:, w:] == 0).all()                             # zero padding
        assert not covered[off:off + H * Wp].any()
        covered[off:off + H * Wp] = True
        end = off + H * Wp
    assert end <= flat.size and (flat[~covered] == 0).all()
    # a staging buffer is used when it is large enough (same layout)
    stage = torch.full((end + 100,), 7.0)
    pf2 = pack_frames([np.asarray(m) for m in maps], device="cpu", pinned=stage)
    np.testing.assert_array_equal(pf2.depth.numpy(), flat[:pf2.depth.numel()])
    assert pf2.depth.data_ptr() == stage.data_ptr()
    with pytest.raises(ValueError, match="must be \\(H, W\\)"):
        pack_frames([np.zeros((2, 3, 4), np.float32)], device="cpu")
    with pytest.raises(ValueError, match="empty frame"):
        pack_frames([np.zeros((0, 4), np.float32)], device="cpu")
    empty = pack_frames([], device="cpu")
    assert tuple(empty.table.shape) == (0, 6) and empty.sizes == []


def _cpu_frames():
    from labelany3d_amd import pack_frames

    return pack_frames([np.ones((8, 32), np.float32), np.ones((16, 64), np.float32)], device="cpu")


def test_argument_errors_come_before_device_work():
    """every error below is raised on a machine without a GPU: nothing has touched a device when it comes"""
    from labelany3d_amd import fit_instances_frames

    pf = _cpu_frames()
    K = np.eye(3)
    rles = [{"size": [8, 32], "counts": [0, 256]}]
    with pytest.raises(ValueError, match="convex_hull"):
        fit_instances_frames(pf, K, rles=rles, image_index=[0], method="convex_hull")
    with pytest.raises(ValueError, match="Unknown method"):
        fit_instances_frames(pf, K, rles=rles, image_index=[0], method="obb")
    with pytest.raises(ValueError, match="exactly one of rles / polys"):
        fit_instances_frames(pf, K, image_index=[0])
    with pytest.raises(ValueError, match="exactly one of rles / polys"):
        fit_instances_frames(pf, K, rles=rles, polys=(np.zeros((1, 2), np.int32), np.zeros(2, np.int64), np.zeros(2, np.int64)), image_index=[0])
    with pytest.raises(ValueError, match="image_index is required"):
        fit_instances_frames(pf, K, rles=rles)
    with pytest.raises(ValueError, match="PackedFrames"):
        fit_instances_frames((pf.depth, pf.table), K, rles=rles, image_index=[0])
    with pytest.raises(ValueError, match="on the GPU"):
        fit_instances_frames(pf, K, rles=rles, image_index=[0])


def test_c_entry_refuses_before_any_launch():
    """the call-level refusals of the C entry, with host pointers that are never dereferenced: they return before a kernel is launched"""
    from labelany3d_amd import _lib

    lib = _lib.lib
    buf = (C.c_double * 64)()
    p = C.addressof(buf)

    def args(**kw):
        a = _lib.FitArgs(struct_size=C.sizeof(_lib.FitArgs), B=1, H=8, W=32, depth=p, K=p, out=p, status=p, workspace=p, image_index=p)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def call(a, frames=p, P=1):
        return lib.la3d_fit_instances_frames(C.byref(a), frames, P), lib.la3d_last_error().decode()

    rc, msg = call(args(mask=p))
    assert rc == _lib.ERR_UNSUPPORTED and "u8 mask planes" in msg
    rc, msg = call(args(rle_counts=p, rle_offsets=p, method=_lib.METHOD_CONVEX_HULL))
    assert rc == _lib.ERR_UNSUPPORTED and "CONVEX_HULL" in msg
    rc, msg = call(args())
    assert rc == -1 and "exactly one of rle_counts / poly_xy" in msg
    rc, msg = call(args(rle_counts=p, rle_offsets=p, image_index=None))
    assert rc == -1 and "image_index is required" in msg
    rc, msg = call(args(rle_counts=p, rle_offsets=p, depth_plane_stride=256))
    assert rc == -1 and "must be 0" in msg
    rc, msg = call(args(rle_counts=p, rle_offsets=p, frame_width=30))
    assert rc == -1 and "must be 0" in msg
    rc, msg = call(args(rle_counts=p, rle_offsets=p), frames=None)
    assert rc == -1 and "frames must be" in msg
    rc, msg = call(args(rle_counts=p, rle_offsets=p), P=0)
    assert rc == -1 and "frames must be" in msg
    rc, msg = call(args(rle_counts=p, rle_offsets=p, depth=p + 4))
    assert rc == -1 and "16-byte aligned" in msg
    rc, msg = call(args(poly_xy=p))
    assert rc == -1 and "ring_offsets" in msg
    rc, msg = call(args(rle_counts=p, rle_offsets=p, H=2048, W=1024))      # beyond the bit image a workgroup's LDS holds
    assert rc == _lib.ERR_UNSUPPORTED and "bit image in LDS" in msg
    rc, msg = call(args(rle_counts=p, rle_offsets=p, struct_size=8))
    assert rc == -1 and "struct_size" in msg
    assert call(args(rle_counts=p, rle_offsets=p, B=0))[0] == 0            # an empty batch is a success, as for every entry


def _scene(i, h, w):
    return {"name": f"s{i}", "height": h, "width": w, "annotations": []}


def test_mixed_batches_keep_arrival_order():
    """``_batches`` with ``mixed_frames``: sizes mix, order is the arrival order, ``batch_images`` per batch; off: keyed by size as before"""
    from labelany3d_amd.fit_scenes import ScenePipeline

    sizes = [(480, 640), (427, 640), (480, 640), (375, 500), (640, 480), (480, 640), (333, 500), (427, 640), (480, 640), (96, 224), (480, 640)]
    scenes = [_scene(i, h, w) for i, (h, w) in enumerate(sizes)]
    pipe = ScenePipeline.__new__(ScenePipeline)        # (batching needs no device: only the two attributes below)
    pipe.batch_images, pipe.mixed_frames = 4, True
    got = list(pipe._batches(iter(scenes)))
    assert [[sc["name"] for sc in b] for b in got] == [["s0", "s1", "s2", "s3"], ["s4", "s5", "s6", "s7"], ["s8", "s9", "s10"]]
    assert any(len({(sc["height"], sc["width"]) for sc in b}) > 1 for b in got)
    pipe.mixed_frames = False
    got = list(pipe._batches(iter(scenes)))
    assert all(len({(sc["height"], sc["width"]) for sc in b}) == 1 for b in got)
    assert [sc["name"] for sc in got[0]] == ["s0", "s2", "s5", "s8"] and sorted(sc["name"] for b in got for sc in b) == sorted(sc["name"] for sc in scenes)
    import inspect
    assert inspect.signature(ScenePipeline.__init__).parameters["mixed_frames"].default is False
