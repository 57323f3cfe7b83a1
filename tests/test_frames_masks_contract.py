"""CPU-only contract of network masks and logits in the frames call (include/la3d.h "images of different sizes in one call":
``la3d_pack_mask_bits_frames``, ``la3d_pack_logits_bits_frames``): the exports exist on every layer, ``pack_mask_frames`` lays the
stacks out dense, in row order, under the table ``pack_frames`` gives depth maps of the same sizes, the argument errors come before
any device work, the C entries refuse before any launch, and the inputs of tests/test_gpu_frames_masks.py are fitted by the oracle
as planned."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import frames_masks_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_C = ("la3d_pack_mask_bits_frames", "la3d_pack_logits_bits_frames")
NEW_PY = ("PackedMasks", "pack_mask_frames", "pack_mask_bits_frames", "fit_instances_frames_masks")


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


def _stacks(dtype, rs):
    """the stacks of case 0 in one dtype -> (what a caller holds, the same as NumPy arrays of the stored element)"""
    import torch

    case = MC.make_case(0)
    if dtype in ("bool", "u8"):
        held = [s if dtype == "bool" else MC.as_u8(s, rs) for s in case["stacks"]]
        return list(held), [h.view(np.uint8) for h in held]
    logits = [MC.as_logits(s, 0.5, rs)[0] for s in case["stacks"]]
    if dtype == "f32":
        return list(logits), list(logits)
    if dtype == "f16":
        held = [x.astype(np.float16) for x in logits]
        return list(held), [h.view(np.int16) for h in held]
    held = [torch.as_tensor(x).to(torch.bfloat16) for x in logits]
    return held, [h.view(torch.int16).numpy() for h in held]


@pytest.mark.parametrize("dtype", ["bool", "u8", "f32", "f16", "bf16"])
def test_pack_mask_frames_layout(dtype):
    import torch

    from labelany3d_amd import _lib, frame_bits_offsets, pack_frames, pack_mask_frames
    from labelany3d_amd.masks import MASKS_U8

    held, want = _stacks(dtype, np.random.RandomState(3))
    if dtype != "bf16":
        held[2] = torch.as_tensor(held[2])                                   # arrays and tensors mix
    pm = pack_mask_frames(held, device="cpu")
    pf = pack_frames([np.ones(s, np.float32) for s in MC.SIZES], device="cpu")
    kind = {"bool": MASKS_U8, "u8": MASKS_U8, "f32": _lib.DTYPE_F32, "f16": _lib.DTYPE_F16, "bf16": _lib.DTYPE_BF16}[dtype]
    store = {"bool": torch.uint8, "u8": torch.uint8, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dtype]
    assert pm.kind == kind and pm.data.dtype == store and pm.data.dim() == 1 and pm.pitch is None
    assert pm.sizes == list(MC.SIZES) and (pm.H, pm.W) == (pf.H, pf.W) == (120, 512)
    np.testing.assert_array_equal(pm.table_host, pf.table_host)             # ONE table serves the packer and the fit
    np.testing.assert_array_equal(pm.table.numpy(), pf.table.numpy())
    flat = pm.data.view(torch.int16).numpy() if dtype in ("f16", "bf16") else pm.data.numpy()
    flat = flat.view(want[0].dtype) if flat.dtype != want[0].dtype else flat
    ii, offs = pm.image_index.numpy(), pm.offsets.numpy()
    assert pm.image_index.dtype == torch.int32 and pm.offsets.dtype == torch.int64
    np.testing.assert_array_equal(ii, np.repeat(np.arange(len(want)), [len(w) for w in want]))   # row order = image order
    planes = [pl for w in want for pl in w]
    at = 0
    for n, pl in enumerate(planes):                                          # dense, back to back: no padding of rows or planes
        assert offs[n] == at and pl.shape == MC.SIZES[ii[n]]
        np.testing.assert_array_equal(flat[at:at + pl.size].reshape(pl.shape), pl)
        at += pl.size
    assert not (ii == MC.NO_MASKS).any()
    boffs, words = frame_bits_offsets(pm.table_host, ii)
    np.testing.assert_array_equal(pm.bits_offsets.numpy(), boffs)
    assert pm.bits_words == words


def test_argument_errors_come_before_device_work():
    """every error below is raised on a machine without a GPU: nothing has touched a device when it comes"""
    import torch

    from labelany3d_amd import fit_instances_frames_masks, pack_frames, pack_mask_bits_frames, pack_mask_frames

    ok = np.zeros((2, 8, 32), np.uint8)
    with pytest.raises(ValueError, match="stack 1 .*another dtype"):
        pack_mask_frames([ok, np.zeros((1, 16, 64), np.float32)], device="cpu")
    with pytest.raises(ValueError, match="stack 1 .*must be \\(N, H, W\\)"):
        pack_mask_frames([ok, np.zeros((16, 64), np.uint8)], device="cpu")
    with pytest.raises(ValueError, match="stack 1 .*empty frame"):
        pack_mask_frames([ok, np.zeros((3, 0, 64), np.uint8)], device="cpu")
    with pytest.raises(ValueError, match="stack 0 .*must be bool, uint8"):
        pack_mask_frames([np.zeros((2, 8, 32), np.int32)], device="cpu")
    with pytest.raises(ValueError, match="stack 1 .*another dtype"):
        pack_mask_frames([torch.zeros((2, 8, 32), dtype=torch.float16), torch.zeros((1, 16, 64), dtype=torch.bfloat16)], device="cpu")
    sizes = [(8, 32), (16, 64)]
    pf = pack_frames([np.ones(s, np.float32) for s in sizes], device="cpu")
    stacks = [np.zeros((2,) + sizes[0], bool), np.zeros((0,) + sizes[1], bool)]
    K = np.eye(3)
    with pytest.raises(ValueError, match="fit_instances_frames_masks: method='convex_hull' is not supported for frames of different sizes"):
        fit_instances_frames_masks(pf, stacks, K, method="convex_hull")
    with pytest.raises(ValueError, match="Unknown method"):
        fit_instances_frames_masks(pf, stacks, K, method="obb")
    with pytest.raises(ValueError, match="height_rule"):
        fit_instances_frames_masks(pf, stacks, K, height_rule="tall")
    with pytest.raises(ValueError, match="another \\(H, W\\)"):
        fit_instances_frames_masks(pf, [stacks[0], np.zeros((1, 16, 40), bool)], K)
    with pytest.raises(ValueError, match="another \\(H, W\\)"):
        fit_instances_frames_masks(pf, stacks[:1], K)
    pm = pack_mask_frames(stacks, device="cpu")
    with pytest.raises(ValueError, match="another \\(H, W\\)"):
        fit_instances_frames_masks(pack_frames([np.ones((8, 32), np.float32), np.ones((16, 40), np.float32)], device="cpu"), pm, K)
    with pytest.raises(ValueError, match="on the GPU"):
        pack_mask_bits_frames(pm)
    with pytest.raises(ValueError, match="on the GPU"):
        fit_instances_frames_masks(pf, pm, K)


def test_c_packers_refuse_before_any_launch():
    """the call-level refusals of both entries, with host pointers that are never dereferenced and a NULL stream"""
    from labelany3d_amd import _lib

    lib = _lib.lib
    buf = (C.c_double * 64)()
    p = (C.addressof(buf) + 15) & ~15

    def u8(src=p, frames=p, P=1, H=8, W=32, ii=p, soffs=p, pit=None, B=1, bits=p, boffs=p, area=None):
        rc = lib.la3d_pack_mask_bits_frames(src, frames, P, H, W, ii, soffs, pit, B, bits, boffs, area, None)
        return rc, lib.la3d_last_error().decode()

    def lg(src=p, dtype=_lib.DTYPE_F16, thr=0.0, frames=p, P=1, H=8, W=32, ii=p, soffs=p, pit=None, B=1, bits=p, boffs=p, area=None):
        rc = lib.la3d_pack_logits_bits_frames(src, dtype, thr, frames, P, H, W, ii, soffs, pit, B, bits, boffs, area, None)
        return rc, lib.la3d_last_error().decode()

    for dtype in (3, 7, -1):                                                 # (3: LA3D_DTYPE_U16 is a depth dtype, no logit)
        rc, msg = lg(dtype=dtype)
        assert rc == -1 and "la3d_pack_logits_bits_frames: unknown dtype" in msg
    for call, who in ((u8, "la3d_pack_mask_bits_frames"), (lg, "la3d_pack_logits_bits_frames")):
        for kw in (dict(B=-1), dict(P=-1), dict(H=0), dict(W=0), dict(H=-3)):
            rc, msg = call(**kw)
            assert rc == -1 and msg.startswith(who) and "bad argument" in msg, kw
        rc, msg = call(H=1 << 15, W=1 << 15)                                  # bounds beyond H * roundup32(W) <= 2^28
        assert rc == -1 and "too large" in msg
        rc, msg = call(H=1 << 14, W=1 << 14, B=1 << 17)                       # B * chunks >= 2^31 (chunks = 2^15)
        assert rc == -1 and "too large" in msg
        assert call(H=1 << 14, W=1 << 14, B=0)[0] == 0
        for name in ("src", "frames", "ii", "soffs", "bits", "boffs"):
            rc, msg = call(**{name: None})
            assert rc == -1 and "NULL" in msg, name
        rc, msg = call(bits=p + 2)
        assert rc == -1 and "4-byte aligned" in msg
        for name in ("frames", "soffs", "boffs"):
            rc, msg = call(**{name: p + 4})
            assert rc == -1 and "8-byte aligned" in msg, name
        for name in ("ii", "pit", "area"):
            rc, msg = call(**{name: p + 2})
            assert rc == -1 and "4-byte aligned" in msg, name
        assert call(B=0)[0] == 0 and call(P=0)[0] == 0                        # nothing to do: success
        assert call(B=0, src=None, frames=None, bits=None)[0] == 0
    assert u8(src=p + 1, B=0)[0] == 0                                         # (any byte address holds a u8 mask)
    rc, msg = lg(src=p + 1)
    assert rc == -1 and "element size" in msg
    rc, msg = lg(src=p + 2, dtype=_lib.DTYPE_F32)
    assert rc == -1 and "element size" in msg
    rc, msg = lg(src=p + 1, dtype=_lib.DTYPE_BF16)
    assert rc == -1 and "element size" in msg


@pytest.mark.parametrize("seed", MC.SEEDS)
def test_the_gpu_cases_are_fitted_by_the_oracle_as_planned(seed):
    """every instance that is not there for its status has status 0, the two special ones 1 and 3; 2 - 5 instances per image, one
    image without, and the run lengths decode to the masks"""
    from oracle import la3d_oracle as O

    from .test_gpu_frames import oracle_mix

    case = MC.make_case(seed)
    rec, st, yaw, nv = oracle_mix(case)
    np.testing.assert_array_equal(st, case["expect"])
    assert sorted(case["expect"][case["expect"] != 0].tolist()) == [1, 3]
    assert np.isfinite(rec[st == 0]).all()
    per = np.bincount(case["img"], minlength=len(MC.SIZES))
    assert per[MC.NO_MASKS] == 0 and case["stacks"][MC.NO_MASKS].shape == (0,) + MC.SIZES[MC.NO_MASKS]
    plain = per - (np.arange(len(per)) == MC.EMPTY_IMAGE) - (np.arange(len(per)) == MC.PIXEL_IMAGE)
    assert ((plain >= 2) & (plain <= 5))[np.arange(len(per)) != MC.NO_MASKS].all()
    assert sorted(case["order"].tolist()) == list(range(len(case["img"]))) and (np.diff(case["img"][case["order"]]) < 0).any()
    for m, r, p, e in zip(case["masks"], case["rles"], case["img"], case["expect"]):
        assert m.shape == MC.SIZES[p] and m.dtype == bool
        np.testing.assert_array_equal(O.rle_decode(r["counts"], *r["size"]), m)
        assert m.sum() == {1: 0, 3: 1}.get(int(e), m.sum())
    np.testing.assert_array_equal(np.concatenate([s.reshape(-1) for s in case["stacks"]]), np.concatenate([m.reshape(-1) for m in case["masks"]]))
