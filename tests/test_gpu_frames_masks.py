"""Network masks and logits of images of different sizes in one call (include/la3d.h "images of different sizes in one call":
la3d_pack_mask_bits_frames, la3d_pack_logits_bits_frames) on the GPU: the packer bit for bit against np.packbits for every element
kind, the planes read where they lie (no copy, a crop of a canvas among them), the fit against the run-length frames call of the same
masks (bit for bit: the same engine on the same bit image) and against the oracle, the on-device refusals, and pack + fit captured
into a graph.  The inputs (tests/frames_masks_cases.py) are checked on the oracle alone by tests/test_frames_masks_contract.py."""
import ctypes as C

import numpy as np
import pytest

from . import frames_masks_cases as MC
from .test_gpu_frames import ground_rows, np_, oracle_mix
from .test_gpu_frames_bits import KEYS, SENTINEL, check_fit, trio

pytestmark = pytest.mark.gpu

DTYPES = ("u8", "bool", "f32", "f16", "bf16")


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


_REF = {}


def case_and_ref(seed, **kw):
    """a case and the oracle's answer for it, computed once and shared (never written to)"""
    key = (seed,) + tuple(sorted(kw))
    if key not in _REF:
        case = MC.make_case(seed)
        _REF[key] = (case, oracle_mix(case, **{k: v(case) for k, v in kw.items()}))
    return _REF[key]


def held_stacks(case, dtype, threshold, seed=5):
    """the stacks of a case as a caller holds them in one dtype (host: NumPy, bfloat16: torch) -> (stacks, the masks they mean, row by
    row in image order)"""
    import torch

    rs = np.random.RandomState(seed)
    if dtype == "bool":
        return list(case["stacks"]), case["masks"]
    if dtype == "u8":
        return [MC.as_u8(s, rs) for s in case["stacks"]], case["masks"]
    pairs = [MC.as_logits(s, threshold, rs) for s in case["stacks"]]
    mean = [m for _, ms in pairs for m in ms]
    if dtype == "f32":
        return [x for x, _ in pairs], mean
    if dtype == "f16":
        return [x.astype(np.float16) for x, _ in pairs], mean
    return [torch.as_tensor(x).to(torch.bfloat16) for x, _ in pairs], mean


def check_planes(fb, out, mean, img, offsets, total, tag):
    """every plane holds np.packbits of its mask on rows zero-padded to the pitch; every other word keeps the sentinel; area = popcount"""
    buf = np_(out).view(np.uint32)
    want = np.full(buf.shape, SENTINEL, np.uint32)
    for b, w in enumerate(MC.expected_words(mean)):
        want[offsets[b]:offsets[b] + len(w)] = w
    np.testing.assert_array_equal(np_(fb.offsets), offsets, err_msg=f"{tag} offsets")
    np.testing.assert_array_equal(buf[:total], want[:total], err_msg=f"{tag} words")
    assert (buf[total:] == SENTINEL).all(), f"{tag}: words behind the last plane were written"
    np.testing.assert_array_equal(np_(fb.area), [m.sum() for m in mean], err_msg=f"{tag} area")
    np.testing.assert_array_equal(np_(fb.image_index), img, err_msg=f"{tag} image_index")


# ------------------------------------------------------------------------------------------
# 1. the packer, bit for bit
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,threshold", [("u8", 0.0), ("bool", 0.0)] + [(d, t) for d in ("f32", "f16", "bf16") for t in (0.0, 0.5)])
def test_packer_equals_packbits(la, dtype, threshold):
    import torch

    case = MC.make_case(1)
    stacks, mean = held_stacks(case, dtype, threshold)
    img = case["img"]
    pm = la.pack_mask_frames(stacks)                                          # host stacks: dense, back to back, one upload
    assert pm.pitch is None and not pm.sources and pm.data.is_cuda
    offsets, total = la.frame_bits_offsets(pm.table_host, img)
    words = np.asarray([MC.SIZES[p][0] * MC.FC.pitch(MC.SIZES[p][1]) // 32 for p in img], np.int64)
    assert {150, 14} <= set(words.tolist()) and ((words + 3) // 4 * 4 != words).any()      # some planes leave a gap for the sentinel
    es = pm.data.element_size()
    lies = (pm.data.data_ptr() + np_(pm.offsets) * es) % 16
    assert (lies == 0).any() and (lies != 0).any()                            # planes on and off a 16-byte boundary in one launch
    out = torch.full((total + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    fb = la.pack_mask_bits_frames(pm, threshold=threshold, out=out)
    assert fb.bits.data_ptr() == out.data_ptr() and (fb.H, fb.W) == (pm.H, pm.W) == (120, 512)
    check_planes(fb, out, mean, img, offsets, total, f"{dtype} thr {threshold}")
    # the rows in another order (image_index no longer sorted): every plane follows its row
    order = case["order"]
    t = torch.as_tensor(order, device="cuda")
    offs2, total2 = la.frame_bits_offsets(pm.table_host, img[order])
    shuffled = pm._replace(offsets=pm.offsets[t].contiguous(), image_index=pm.image_index[t].contiguous(),
                           bits_offsets=torch.as_tensor(offs2, device="cuda"), bits_words=total2)
    out2 = torch.full((total2 + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    fb2 = la.pack_mask_bits_frames(shuffled, threshold=threshold, out=out2)
    check_planes(fb2, out2, [mean[i] for i in order], img[order], offs2, total2, f"{dtype} thr {threshold} shuffled")
    # a sequence goes through pack_mask_frames; without out=: the same words
    fb3 = la.pack_mask_bits_frames(stacks, threshold=threshold)
    got = np_(fb3.bits).view(np.uint32)
    for b, w in enumerate(MC.expected_words(mean)):
        np.testing.assert_array_equal(got[offsets[b]:offsets[b] + len(w)], w)


# ------------------------------------------------------------------------------------------
# 2. device tensors are read where they lie
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["u8", "bool", "f16", "f32"])
def test_device_stacks_are_read_in_place(la, dtype):
    """separate device tensors, one of them the top-left crop of a canvas that is set / above the threshold everywhere outside the
    crop (pitch 96 > 75 image columns: whole 16-byte groups reach past the image columns, and in the last row must not), one a slice
    that starts one element into its allocation (off every 16-byte boundary): nothing is copied, and the words are those of test 1"""
    import torch

    threshold = 0.5
    case = MC.make_case(1)
    stacks, mean = held_stacks(case, dtype, threshold)
    dev = []
    for p, s in enumerate(stacks):
        s = s if isinstance(s, np.ndarray) else s.numpy()
        if p == MC.CANVAS_IMAGE:
            fill = True if dtype == "bool" else 255 if dtype == "u8" else np.inf
            canvas, _ = MC.canvas_of(s, fill)
            t = torch.as_tensor(canvas, device="cuda")
            h, w = MC.SIZES[p]
            dev.append(t[:, :h, :w])
            assert not dev[-1].is_contiguous() and dev[-1].stride(1) == w + MC.CANVAS_EXTRA[1] == 96
        elif p == 4:
            whole = torch.zeros(s.size + 1, dtype=torch.as_tensor(s[:0]).dtype, device="cuda")
            whole[1:] = torch.as_tensor(s.reshape(-1), device="cuda")
            dev.append(whole[1:].view(s.shape))
        else:
            dev.append(torch.as_tensor(s, device="cuda"))
    pm = la.pack_mask_frames(dev)
    live = [t for t in dev if t.shape[0]]
    low = min(t.data_ptr() for t in live)
    es = pm.data.element_size()
    assert pm.data.data_ptr() == low and len(pm.sources) == len(live)        # no copy: data aliases the lowest source
    addressed = pm.data.data_ptr() + np_(pm.offsets) * es                     # what the call addresses, row by row
    want = np.concatenate([t.data_ptr() + np.arange(t.shape[0]) * t.stride(0) * es for t in live])
    np.testing.assert_array_equal(addressed, want)
    pitch = np_(pm.pitch)
    np.testing.assert_array_equal(pitch, [96 if p == MC.CANVAS_IMAGE else MC.SIZES[p][1] for p in case["img"]])
    offsets, total = la.frame_bits_offsets(pm.table_host, case["img"])
    out = torch.full((total + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    fb = la.pack_mask_bits_frames(pm, threshold=threshold, out=out)
    check_planes(fb, out, mean, case["img"], offsets, total, f"{dtype} in place")


# ------------------------------------------------------------------------------------------
# 3. the fit: bit for bit the run-length frames call, and the oracle
# ------------------------------------------------------------------------------------------
def identical(got, other, tag, keys=KEYS):
    for k in keys:
        np.testing.assert_array_equal(np.nan_to_num(np_(got[k]), nan=-7.0), np.nan_to_num(np_(other[k]), nan=-7.0), err_msg=f"{tag} {k}")


@pytest.mark.parametrize("seed", MC.SEEDS)
@pytest.mark.parametrize("dtype", ["bool", "f16"])
def test_fit_equals_the_run_length_call_and_the_oracle(la, seed, dtype):
    case, ref = case_and_ref(seed)
    np.testing.assert_array_equal(ref[1], case["expect"])                    # (on the CPU, first)
    stacks, mean = held_stacks(case, dtype, 0.0)
    if dtype != "bool":                                                      # (the logits' NaN / inf pixels change the masks: fit the plain ones)
        stacks = [np.where(s, 1.0, -1.0).astype(np.float16) for s in case["stacks"]]
    pf = la.pack_frames(case["depth"])
    res = la.fit_instances_frames_masks(pf, stacks, case["K"], proj=True)
    fb = res["bits"]
    np.testing.assert_array_equal(np_(fb.image_index), case["img"])
    np.testing.assert_array_equal(np_(fb.area), [m.sum() for m in case["masks"]])
    rle = la.fit_instances_frames(pf, case["K"], rles=case["rles"], image_index=case["img"], proj=True)
    identical(res, rle, f"seed {seed} {dtype}", KEYS + ("boxes2d",))
    check_fit(res, case, ref, f"seed {seed} {dtype}")
    assert set(np_(res["status"]).tolist()) == {0, 1, 3}


@pytest.mark.parametrize("variant", ["ground", "sample", "u16"])
def test_fit_variants(la, variant):
    case, plain = case_and_ref(0)
    B = len(case["img"])
    u8 = [MC.as_u8(s, np.random.RandomState(2)) for s in case["stacks"]]
    pf = la.pack_frames(case["depth"])
    if variant == "ground":
        g = ground_rows(B, 5)
        case, ref = case_and_ref(0, ground=lambda c: g)
        res = la.fit_instances_frames_masks(pf, u8, case["K"], ground=g)
        identical(res, la.fit_instances_frames(pf, case["K"], rles=case["rles"], image_index=case["img"], ground=g), "ground")
        check_fit(res, case, ref, "ground")
    elif variant == "sample":
        areas = np.asarray([m.sum() for m in case["masks"]])
        assert (areas > 500).any() and (areas <= 500).any()                  # both sides of the reference's subsample rule
        sidx = la.draw_sample_idx(areas, np.random.RandomState(9))
        case, ref = case_and_ref(0, sidx=lambda c: sidx)
        res = la.fit_instances_frames_masks(pf, u8, case["K"], sample_idx=sidx)
        identical(res, la.fit_instances_frames(pf, case["K"], rles=case["rles"], image_index=case["img"], sample_idx=sidx), "subsample")
        check_fit(res, case, ref, "subsample")
    else:
        scale = np.float32(0.001)
        stored = [np.rint(d / scale).astype(np.uint16) for d in case["depth"]]
        for s in stored:
            s[::5, ::7] = 0                                                  # holes under the masks
        up = [np.where(s == 0, np.float32(np.nan), s.astype(np.float32) * scale).astype(np.float32) for s in stored]
        pf16 = la.pack_frames(stored, dtype="u16", scale=0.001, zero_is_hole=True)
        assert isinstance(pf16, la.PackedFrames16)
        res = la.fit_instances_frames_masks(pf16, u8, case["K"], proj=True)
        identical(res, la.fit_instances_frames(pf16, case["K"], rles=case["rles"], image_index=case["img"], proj=True), "u16 depth",
                  KEYS + ("boxes2d",))
        case16 = dict(case, depth=up)
        check_fit(res, case16, oracle_mix(case16), "u16 depth")


# ------------------------------------------------------------------------------------------
# 4. broken rows through the C entry, every array on the device
# ------------------------------------------------------------------------------------------
def test_broken_rows_are_left_or_zeroed_and_the_fit_refuses_them(la):
    """No address is ever formed from a broken value - the kernel tests image_index, the frame row and bits_offsets before it forms the
    output address, and src_offsets / pitch before it forms a source address (pack_masks_frames_kernel) - so this test does not rest
    on a fault: it checks what the planes and the sentinel around them hold afterwards."""
    import torch

    from labelany3d_amd import _lib

    case, ref = case_and_ref(0)
    img, B, P = case["img"], len(case["img"]), len(MC.SIZES)
    u8 = [MC.as_u8(s, np.random.RandomState(4)) for s in case["stacks"]]
    pf = la.pack_frames(case["depth"])
    pm = la.pack_mask_frames(u8)
    BROKEN = 4                                                               # image 4 gets a pitch of 33, in the packer's table and the fit's
    for tab in (pf.table, pm.table):
        tab[BROKEN, 3] = 33
    rows4 = np.flatnonzero(img == BROKEN)
    minus, beyond = int(np.flatnonzero(img == 0)[0]), int(np.flatnonzero(img == 5)[0])
    two, negsrc, narrow = int(np.flatnonzero(img == 0)[2]), int(np.flatnonzero(img == 6)[1]), int(np.flatnonzero(img == 1)[0])
    offs_h, total = la.frame_bits_offsets(pm.table_host, img)
    ii_bad, boffs_bad, soffs_bad = img.copy(), offs_h.copy(), np_(pm.offsets).copy()
    pitch = np.asarray([MC.SIZES[p][1] for p in img], np.int32)
    ii_bad[minus], ii_bad[beyond] = -1, P
    boffs_bad[two] = 2
    soffs_bad[negsrc] = -5
    pitch[narrow] -= 1
    kept = np.zeros(B, bool)
    kept[rows4] = kept[[minus, beyond, two]] = True
    zeroed = np.zeros(B, bool)
    zeroed[[negsrc, narrow]] = True
    assert (kept | zeroed).sum() == len(rows4) + 5 and (case["expect"][kept | zeroed] == 0).all()
    MARGIN = 4096                                                            # a write through a small wrong offset would land in the sentinel
    whole = torch.full((MARGIN + total + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
    bits = whole[MARGIN:]
    ii, boffs, soffs, pit = (torch.as_tensor(a, device="cuda") for a in (ii_bad, boffs_bad, soffs_bad, pitch))
    area = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = _lib.lib.la3d_pack_mask_bits_frames(ptr(pm.data), ptr(pm.table), P, pm.H, pm.W, ptr(ii), ptr(soffs), ptr(pit), B, ptr(bits), ptr(boffs),
                                             ptr(area), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib.la3d_last_error()
    torch.cuda.synchronize()
    want = np.full(whole.numel(), SENTINEL, np.uint32)
    want_area = np.zeros(B, np.int64)
    for b, w in enumerate(MC.expected_words(case["masks"])):
        if zeroed[b]:
            want[MARGIN + offs_h[b]:MARGIN + offs_h[b] + len(w)] = 0
        elif not kept[b]:
            want[MARGIN + offs_h[b]:MARGIN + offs_h[b] + len(w)] = w
            want_area[b] = case["masks"][b].sum()
    np.testing.assert_array_equal(np_(whole).view(np.uint32), want, err_msg="a refused row was written, an unreadable one not zeroed, or a conforming one missed")
    np.testing.assert_array_equal(np_(area), want_area)
    fb = la.FrameBits(bits, boffs, ii, area, pm.table_host, pm.H, pm.W)
    res = la.fit_instances_frames_bits(pf, fb, case["K"], proj=True)
    boxes, status, aux = trio(res)
    np.testing.assert_array_equal(status[kept], 5)
    np.testing.assert_array_equal(status[zeroed], 1)
    assert np.isnan(boxes[kept | zeroed]).all() and np.isnan(np_(res["boxes2d"])[kept | zeroed]).all()
    check_fit(res, case, ref, "the others", sel=np.flatnonzero(~(kept | zeroed)))


# ------------------------------------------------------------------------------------------
# 5. pack + fit captured into a graph
# ------------------------------------------------------------------------------------------
def test_masks_call_captured_into_a_graph(la):
    """resident depth, masks and K: pack + fit are a chain on one stream, captured once and replayed once"""
    import torch

    dev = torch.device("cuda", 0)
    case = MC.make_case(2)
    pf = la.pack_frames(case["depth"])
    pm = la.pack_mask_frames(case["stacks"])
    K = torch.as_tensor(case["K"], device=dev)
    eager = la.fit_instances_frames_masks(pf, pm, K)
    want = trio(eager)
    side = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        la.fit_instances_frames_masks(pf, pm, K, stream=side)                # (warm-up: every small upload is cached)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            res = la.fit_instances_frames_masks(pf, pm, K, stream=torch.cuda.current_stream())
    g.replay()
    torch.cuda.synchronize()
    for a, b, k in zip(trio(res), want, KEYS):
        np.testing.assert_array_equal(np.nan_to_num(a, nan=-7.0), np.nan_to_num(b, nan=-7.0), err_msg=k)
    np.testing.assert_array_equal(np_(res["bits"].area), [m.sum() for m in case["masks"]])
    assert (np_(res["status"]) == case["expect"]).all()
