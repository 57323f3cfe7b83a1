"""CPU-only contract of label maps and bit planes in the frames call (include/la3d.h "images of different sizes in one call":
``la3d_fit_instances_frames_bits``, ``la3d_pack_label_bits_frames``): the exports exist on every layer, ``pack_label_frames`` lays
label maps out by the table ``pack_frames`` gives depth maps of the same sizes, the plane offsets are aligned and disjoint, the
argument errors come before any device work, the C entries refuse before any launch, and the inputs of
tests/test_gpu_frames_bits.py are fitted by the oracle as planned."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import frames_bits_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_C = ("la3d_fit_instances_frames_bits", "la3d_pack_label_bits_frames")
NEW_PY = ("pack_label_frames", "pack_label_bits_frames", "fit_instances_frames_bits", "fit_instances_frames_labels", "PackedLabels",
          "FrameBits", "frame_bits_offsets")


def test_exports_on_every_layer():
    import labelany3d_amd as la
    from labelany3d_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    for fn in NEW_C:
        assert re.search(rf"\b{fn}\s*\(", hdr), fn
        assert fn in _lib.EXPORTS and hasattr(_lib.lib, fn), fn
    for fn in NEW_PY:
        assert callable(getattr(la, fn)) and fn in la.__all__, fn
    # additive: the ABI version and the argument block stay
    assert re.search(r"#define LA3D_ABI_VERSION 2\b", hdr) and _lib.lib.la3d_version() == 2
    assert C.sizeof(_lib.FitArgs) == 232


def test_pack_label_frames_layout():
    import torch

    from labelany3d_amd import _lib, pack_frames, pack_label_frames

    rs = np.random.RandomState(5)
    sizes = FC.SIZES
    for dt, code in ((np.uint8, _lib.LABEL_U8), (np.uint16, _lib.LABEL_U16), (np.int16, _lib.LABEL_U16), (np.int32, _lib.LABEL_I32)):
        info = np.iinfo(dt)
        maps = [rs.randint(info.min, int(info.max) + 1, s, dtype=np.int64).astype(dt) for s in sizes]
        maps[2] = torch.as_tensor(maps[2].view(np.int16) if dt == np.uint16 else maps[2])   # tensors and arrays mix
        pl = pack_label_frames(maps, device="cpu")
        pf = pack_frames([np.ones(s, np.float32) for s in sizes], device="cpu")
        assert pl.code == code and pl.sizes == list(sizes) and (pl.H, pl.W) == (pf.H, pf.W) == (120, 512)
        np.testing.assert_array_equal(pl.table_host, pf.table_host)          # ONE table serves the packer and the fit
        np.testing.assert_array_equal(pl.table.numpy(), pf.table.numpy())
        flat = pl.data.numpy()
        assert flat.ndim == 1 and flat.dtype == (np.int16 if dt == np.uint16 else dt)
        covered = np.zeros(flat.shape, bool)
        for m, row in zip(maps, pl.table_host):
            off, H, Wp, fw = int(row["depth_offset"]), int(row["H"]), int(row["W"]), int(row["frame_width"])
            plane = flat[off:off + H * Wp].reshape(H, Wp)
            np.testing.assert_array_equal(plane[:, :fw].view(np.asarray(m).dtype), np.asarray(m))
            assert (plane[:, fw:] == 0).all()                                # the padding is zero
            covered[off:off + H * Wp] = True
        assert (flat[~covered] == 0).all()
    # RGB: the same table counted in PIXELS, three bytes each
    rgb = [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in sizes]
    pr = pack_label_frames(rgb, rgb=True, device="cpu")
    assert pr.code == _lib.LABEL_RGB8 and pr.data.dtype == torch.uint8
    np.testing.assert_array_equal(pr.table_host, pf.table_host)
    flat = pr.data.numpy()
    for m, row in zip(rgb, pr.table_host):
        off, H, Wp, fw = int(row["depth_offset"]), int(row["H"]), int(row["W"]), int(row["frame_width"])
        plane = flat[off * 3:(off + H * Wp) * 3].reshape(H, Wp, 3)
        np.testing.assert_array_equal(plane[:, :fw], m)
        assert (plane[:, fw:] == 0).all()
    with pytest.raises(ValueError, match="must be \\(H, W\\)"):
        pack_label_frames([np.zeros((2, 3, 4), np.uint8)], device="cpu")
    with pytest.raises(ValueError, match="rgb=True"):
        pack_label_frames([np.zeros((4, 4), np.uint8)], rgb=True, device="cpu")
    with pytest.raises(ValueError, match="uint8, uint16"):
        pack_label_frames([np.zeros((4, 4), np.float32)], device="cpu")
    with pytest.raises(ValueError, match="one dtype"):
        pack_label_frames([np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.int32)], device="cpu")


def test_plane_offsets_are_aligned_and_disjoint():
    from labelany3d_amd import frame_bits_offsets
    from labelany3d_amd.masks import frame_table

    table = frame_table(FC.SIZES)
    ii = np.array([0, 0, 1, 2, 2, 2, 5, 6, 4, 1, 2], np.int32)             # (unsorted, repeated: the layout follows the rows)
    offs, total = frame_bits_offsets(table, ii)
    words = table["H"].astype(np.int64)[ii] * table["W"][ii] // 32
    assert offs.dtype == np.int64 and (offs % 4 == 0).all() and offs[0] == 0
    assert (offs[1:] >= offs[:-1] + words[:-1]).all() and total >= offs[-1] + words[-1]
    assert (offs[1:] - (offs[:-1] + words[:-1]) < 4).all()                   # and no more than the rounding between two planes
    assert set(words.tolist()) >= {150, 14}                                  # planes that end inside a 16-byte group
    assert frame_bits_offsets(table, [])[1] == 0


def _cpu_inputs():
    import torch

    from labelany3d_amd import FrameBits, pack_frames

    sizes = [(8, 32), (16, 64)]
    pf = pack_frames([np.ones(s, np.float32) for s in sizes], device="cpu")
    fb = FrameBits(torch.zeros(64, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32),
                   torch.zeros(1, dtype=torch.int32), pf.table_host, pf.H, pf.W)
    return pf, fb


def test_argument_errors_come_before_device_work():
    """every error below is raised on a machine without a GPU: nothing has touched a device when it comes"""
    from labelany3d_amd import (Depth16, fit_instances_frames_bits, fit_instances_frames_labels, pack_frames, pack_label_bits_frames,
                                pack_label_frames)

    pf, fb = _cpu_inputs()
    K = np.eye(3)
    with pytest.raises(ValueError, match="convex_hull"):
        fit_instances_frames_bits(pf, fb, K, method="convex_hull")
    with pytest.raises(ValueError, match="Unknown method"):
        fit_instances_frames_bits(pf, fb, K, method="obb")
    with pytest.raises(ValueError, match="height_rule"):
        fit_instances_frames_bits(pf, fb, K, height_rule="tall")
    import torch

    with pytest.raises(ValueError, match="float32 depth planes only"):
        fit_instances_frames_bits(Depth16(torch.zeros((1, 8, 32), dtype=torch.float16)), fb, K)
    with pytest.raises(ValueError, match="PackedFrames"):
        fit_instances_frames_bits((pf.depth, pf.table), fb, K)
    with pytest.raises(ValueError, match="FrameBits"):
        fit_instances_frames_bits(pf, (fb.bits, fb.offsets), K)
    other = pack_frames([np.ones((8, 32), np.float32), np.ones((16, 40), np.float32)], device="cpu")   # same bounds, another table
    assert (other.H, other.W) == (pf.H, pf.W)
    with pytest.raises(ValueError, match="another frame table"):
        fit_instances_frames_bits(other, fb, K)
    with pytest.raises(ValueError, match="on the GPU"):
        fit_instances_frames_bits(pf, fb, K)
    with pytest.raises(ValueError, match="convex_hull"):
        fit_instances_frames_labels(pf, [np.zeros((8, 32), np.uint8), np.zeros((16, 64), np.uint8)], [[1], [2]], K, method="convex_hull")
    pl = pack_label_frames([np.zeros((8, 32), np.uint8), np.zeros((16, 64), np.uint8)], device="cpu")
    with pytest.raises(ValueError, match="one id sequence per image"):
        pack_label_bits_frames(pl, [[1]])
    with pytest.raises(ValueError, match="PackedLabels"):
        pack_label_bits_frames((pl.data, pl.table), [[1], [2]])
    with pytest.raises(ValueError, match="on the GPU"):
        pack_label_bits_frames(pl, [[1], [2]])


def test_label_instances_takes_maps_of_different_sizes():
    from labelany3d_amd import label_instances

    case = FC.make_case(0)
    ids, areas = label_instances(case["maps"], ignore=())
    assert len(ids) == len(FC.SIZES)
    for p, v in enumerate(case["values"]):
        u, c = np.unique(v, return_counts=True)
        np.testing.assert_array_equal(ids[p], u)
        np.testing.assert_array_equal(areas[p], c)
    same = label_instances(np.stack([case["maps"][0]] * 2), ignore=())       # same-shape input: as before
    np.testing.assert_array_equal(same[0][1], ids[0])


def test_c_fit_entry_refuses_before_any_launch():
    """the call-level refusals of la3d_fit_instances_frames_bits, with host pointers that are never dereferenced"""
    from labelany3d_amd import _lib

    lib = _lib.lib
    buf = (C.c_double * 64)()
    p = (C.addressof(buf) + 15) & ~15

    def args(**kw):
        a = _lib.FitArgs(struct_size=C.sizeof(_lib.FitArgs), B=1, H=8, W=32, depth=p, K=p, out=p, status=p, workspace=p, image_index=p)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def d16(**kw):
        d = _lib.Depth16Block(struct_size=C.sizeof(_lib.Depth16Block), dtype=_lib.DTYPE_U16, planes=p, plane_stride=0, scale=0.001, flags=0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(a, depth16=None, frames=p, P=1, bits=p, offsets=p, flags=0):
        rc = lib.la3d_fit_instances_frames_bits(C.byref(a), None if depth16 is None else C.byref(depth16), frames, P, bits, offsets, flags)
        return rc, lib.la3d_last_error().decode()

    for second in (dict(mask=p), dict(rle_counts=p, rle_offsets=p), dict(poly_xy=p, ring_offsets=p, inst_rings=p)):
        rc, msg = call(args(**second))
        assert rc == -1 and "must be NULL" in msg, second
    for bad in (p + 4, p + 8, None):
        rc, msg = call(args(), bits=bad)
        assert rc == -1 and "mask_bits must be a 16-byte aligned" in msg
    rc, msg = call(args(), offsets=None)
    assert rc == -1 and "bits_offsets" in msg
    rc, msg = call(args(), flags=2)
    assert rc == -1 and "bits_flags" in msg
    rc, msg = call(args(method=_lib.METHOD_CONVEX_HULL))
    assert rc == _lib.ERR_UNSUPPORTED and "CONVEX_HULL" in msg
    rc, msg = call(args(image_index=None))
    assert rc == -1 and "image_index is required" in msg
    rc, msg = call(args(depth_plane_stride=256))
    assert rc == -1 and "must be 0" in msg
    rc, msg = call(args(frame_width=30))
    assert rc == -1 and "must be 0" in msg
    rc, msg = call(args(), frames=None)
    assert rc == -1 and "frames must be" in msg
    rc, msg = call(args(depth=p + 4))
    assert rc == -1 and "16-byte aligned" in msg
    rc, msg = call(args(H=2048, W=1024))
    assert rc == _lib.ERR_UNSUPPORTED and "bit image in LDS" in msg
    rc, msg = call(args(struct_size=8))
    assert rc == -1 and "struct_size" in msg
    rc, msg = call(args(opt_engine=99))
    assert rc == -1 and "opt_engine" in msg
    # 16-bit planes: the refusals of the la3d_depth16 block
    rc, msg = call(args(), d16())
    assert rc == -1 and "args->depth must be NULL" in msg
    rc, msg = call(args(depth=None), d16(struct_size=8))
    assert rc == -1 and "struct_size of la3d_depth16" in msg
    rc, msg = call(args(depth=None), d16(dtype=_lib.DTYPE_F32))
    assert rc == -1 and "unknown dtype" in msg
    rc, msg = call(args(depth=None), d16(planes=p + 1))
    assert rc == -1 and "2-byte aligned" in msg
    rc, msg = call(args(depth=None), d16(scale=0.0))
    assert rc == -1 and "scale" in msg
    rc, msg = call(args(depth=None), d16(flags=4))
    assert rc == -1 and "flags" in msg
    rc, msg = call(args(depth=None), d16(dtype=_lib.DTYPE_F16, flags=1))
    assert rc == -1 and "flags must be 0" in msg
    rc, msg = call(args(depth=None), d16(plane_stride=256))
    assert rc == -1 and "plane_stride" in msg
    rc, msg = call(args(depth=None), d16(planes=p + 4))
    assert rc == -1 and "8-byte aligned" in msg
    # an empty batch is a success, as for every entry - with either depth
    assert call(args(B=0))[0] == 0
    assert call(args(B=0, depth=None), d16())[0] == 0
    # and the older frames entry keeps its refusal of bit planes' neighbour, the u8 plane, and its texts
    rc = lib.la3d_fit_instances_frames(C.byref(args(mask=p)), p, 1)
    assert rc == _lib.ERR_UNSUPPORTED and "u8 mask planes" in lib.la3d_last_error().decode()


def test_c_packer_refuses_before_any_launch():
    from labelany3d_amd import _lib

    lib = _lib.lib
    buf = (C.c_double * 64)()
    p = (C.addressof(buf) + 15) & ~15

    def call(labels=p, dtype=_lib.LABEL_U8, frames=p, P=1, H=8, W=32, off=p, lab=p, B=1, bits=p, boffs=p, area=None):
        rc = lib.la3d_pack_label_bits_frames(labels, dtype, frames, P, H, W, off, lab, B, bits, boffs, area, None)
        return rc, lib.la3d_last_error().decode()

    assert call(dtype=7)[0] == -1 and "unknown dtype" in call(dtype=7)[1]
    assert call(H=0)[0] == -1 and call(B=-1)[0] == -1
    rc, msg = call(labels=p + 4)
    assert rc == -1 and "16-byte aligned" in msg
    rc, msg = call(frames=None)
    assert rc == -1 and "NULL" in msg
    rc, msg = call(boffs=p + 4)
    assert rc == -1 and "8-byte aligned" in msg
    rc, msg = call(bits=p + 2)
    assert rc == -1 and "4-byte aligned" in msg
    rc, msg = call(H=1 << 15, W=1 << 15)
    assert rc == -1 and "too large" in msg
    assert call(B=0)[0] == 0 and call(P=0)[0] == 0                            # nothing to do: success


@pytest.mark.parametrize("seed", FC.SEEDS)
def test_the_gpu_cases_are_fitted_by_the_oracle_as_planned(seed):
    """every instance that is not there for its status has status 0, the two special ones 1 and 3 - nothing is filtered or skipped"""
    from .test_gpu_frames import oracle_mix

    case = FC.make_case(seed)
    rec, st, yaw, nv = oracle_mix(case)
    np.testing.assert_array_equal(st, case["expect"])
    assert sorted(case["expect"][case["expect"] != 0].tolist()) == [1, 3] and (case["expect"] == 0).sum() == 30
    assert not (case["img"] == FC.NO_IDS).any() and len(set(case["img"].tolist())) == len(FC.SIZES) - 1
    assert np.isfinite(rec[st == 0]).all()
    # every cell is there, the absent id is absent, the single pixel is single
    for p, v in enumerate(case["values"]):
        assert set(range(1, FC.CELLS + 1)) <= set(np.unique(v).tolist())
        assert not (v == FC.ABSENT_ID).any()
    assert (case["values"][1] == FC.PIXEL_ID).sum() == 1
