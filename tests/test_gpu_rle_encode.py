"""GPU tests of the run-length encoder of bit planes (include/la3d.h "bit planes as run lengths"; ``rle_encode_bits``, ``rle_encode``,
``rle_encode_bits_frames``, ``rle_objects``): the run lists against the CPU oracle's ``rle_encode`` - compared as LISTS, for equality -
on the frame sizes that take every branch of the kernels, the masks whose runs meet the column ends in every way, the plane layouts,
the two-stage protocol (ranges, NO_ROOM, MISMATCH, determinism, graph capture), and the consumers the runs go on to."""
import ctypes as C

import numpy as np
import pytest

from oracle import la3d_oracle as O

from . import frames_fault_rows as FR

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
# (H, W, W_out): the smallest frames that take one branch each - a single pixel; a single row / a single column (the walk of a column
# is one step / there is one column); whole-word rows; H*W % 32 != 0 stored unpadded (a ragged last word, the general bit addressing);
# the same padded to 64 (pad columns); several chunks of words with odd sizes, unpadded and padded; whole 16-byte groups; one VGA frame
FRAMES = [(1, 1, 1), (1, 37, 37), (37, 1, 1), (8, 32, 32), (7, 33, 33), (7, 33, 64), (37, 53, 53), (37, 53, 64), (96, 160, 160), (480, 640, 640)]


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def np_(t):
    return t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()


def mask_set(H, W, seed=0):
    """The masks of one frame, by name: every way a run can meet pixel (0, 0), the last pixel and the column ends."""
    rs = np.random.RandomState(1000 * H + W + seed)
    vv, uu = np.mgrid[0:H, 0:W]
    m = {}
    m["zero"] = np.zeros((H, W), bool)
    m["one"] = np.ones((H, W), bool)
    m["first"] = (vv == 0) & (uu == 0)
    m["last"] = (vv == H - 1) & (uu == W - 1)
    m["checker"] = ((vv + uu) & 1) == 0                                  # the maximum run count (H odd: runs join across columns)
    m["checker_inv"] = ((vv + uu) & 1) == 1
    m["columns"] = (uu & 1) == 1                                         # runs end exactly at column ends
    u = min(W // 2, max(W - 2, 0))
    m["two_columns"] = (uu >= u) & (uu <= u + 1)                         # no transition across the column boundary
    m["across"] = ((uu == u) & (vv == H - 1)) | ((uu == min(u + 1, W - 1)) & (vv == 0))   # one run of 2 across the boundary
    m["row"] = vv == H // 2                                              # W runs of 1
    for d in (0.01, 0.5, 0.99):
        m[f"random{d}"] = rs.rand(H, W) < d
    r = np.zeros((H, W), bool)
    h, w = rs.randint(1, H + 1), rs.randint(1, W + 1)
    r0, c0 = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
    r[r0:r0 + h, c0:c0 + w] = True
    m["rectangle"] = r
    m["rectangle_corner"] = (vv < max(H // 2, 1)) & (uu < max(W // 2, 1))    # a rectangle that holds pixel (0, 0)
    return m


def plane_words(mask, W_out, garbage=False):
    """(H, W) bool -> the uint32 words of its bit plane stored W_out wide; garbage: the pad columns and the spare bits of the last word
    are SET (the encoder must never read them as mask)."""
    H, W = mask.shape
    img = np.full((H, W_out), garbage, bool)
    img[:, :W] = mask
    flat = img.reshape(-1)
    n = (flat.size + 31) // 32 * 32
    flat = np.concatenate([flat, np.full(n - flat.size, garbage, bool)])
    return np.packbits(flat, bitorder="little").view(np.uint32)


def mask_bits(la, masks, W_out, garbage=False, stride_extra=0, misalign=False):
    """A ``MaskBits`` built by hand: planes ``stride_extra`` words further apart than they are long (the gap filled with ones), the base
    4 bytes past a 16-byte boundary with ``misalign``."""
    import torch

    H, W = masks[0].shape
    words = np.stack([plane_words(m, W_out, garbage) for m in masks])
    B, nw = words.shape
    stride = nw + stride_extra
    buf = np.full(B * stride + 8, 0xFFFFFFFF, np.uint32)
    first = 1 if misalign else 0
    rows = buf[first:first + B * stride].reshape(B, stride)
    rows[:, :nw] = words
    t = torch.as_tensor(buf.view(np.int32), device="cuda")
    assert t.data_ptr() % 16 == 0
    planes = t[first:first + B * stride].view(B, stride)
    if stride_extra == 0 and B > 1:
        assert planes.stride(0) == nw
    return la.MaskBits(planes, H, W_out, W)


def split(counts, offsets):
    c, o = np_(counts), np_(offsets)
    return [c[o[i]:o[i + 1]].tolist() for i in range(len(o) - 1)]


def want_of(masks):
    return [O.rle_encode(m)["counts"] for m in masks]


def check_runs(la, mb, masks, tag):
    want = want_of(masks)
    runs, status = la.rle_encode_bits(mb, return_status=True)
    assert isinstance(runs, la.RleRuns) and (runs.H, runs.W) == masks[0].shape, tag
    assert np_(status).tolist() == [0] * len(masks), tag
    np.testing.assert_array_equal(np_(runs.offsets), np.concatenate([[0], np.cumsum([len(w) for w in want])]), err_msg=tag)
    assert runs.counts.numel() == sum(len(w) for w in want), tag
    got = split(runs.counts, runs.offsets)
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{tag}[{n}]: {g[:12]} != {w[:12]}"
    return runs


# ------------------------------------------------------------------------------------------
# 1. values: every frame x every mask
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,W_out", FRAMES, ids=[f"{h}x{w}in{wo}" for h, w, wo in FRAMES])
def test_runs_equal_the_oracle(la, H, W, W_out):
    ms = mask_set(H, W)
    names, masks = list(ms), list(ms.values())
    # garbage: the pad columns of padded rows and the spare bits of a ragged last word are set by hand
    mb = mask_bits(la, masks, W_out, garbage=True)
    runs = check_runs(la, mb, masks, f"{H}x{W} in {W_out} {names}")
    got = dict(zip(names, split(runs.counts, runs.offsets)))
    assert got["zero"] == [H * W] and got["one"] == [0, H * W]
    assert got["first"][0] == 0 and got["last"][-1] == 1
    if W >= 3 and H > 1:
        assert 2 in got["across"]                                            # the one run of 2 that crosses a column end
        assert got["two_columns"] == [c for c in (min(W // 2, W - 2) * H, 2 * H, (W - min(W // 2, W - 2) - 2) * H) if c]
    # the planes of the packer itself (zero padding, frame_pad either way) give the same
    for pad in (True, False):
        check_runs(la, la.pack_mask_bits(np.stack(masks), frame_pad=pad), masks, f"{H}x{W} pack_mask_bits pad={pad}")


@pytest.mark.parametrize("H,W,W_out", [(7, 33, 33), (7, 33, 64), (37, 53, 64), (96, 160, 160)])
@pytest.mark.parametrize("layout", ["stride", "misaligned", "both"])
def test_plane_layouts(la, H, W, W_out, layout):
    """a plane stride larger than a plane; a base aligned to 4 bytes but not to 16 (the word-by-word copy)"""
    masks = list(mask_set(H, W, seed=3).values())
    mb = mask_bits(la, masks, W_out, garbage=True, stride_extra=5 if layout != "misaligned" else 0, misalign=layout != "stride")
    if layout != "stride":
        assert mb.bits.data_ptr() % 16 == 4
    check_runs(la, mb, masks, f"{H}x{W} in {W_out} {layout}")


@pytest.mark.parametrize("B", [1, 300])
def test_batch_sizes(la, B):
    rs = np.random.RandomState(B)
    H, W = 37, 53
    masks = [rs.rand(H, W) < rs.choice([0.02, 0.3, 0.5, 0.97]) for _ in range(B)]
    check_runs(la, mask_bits(la, masks, 64, garbage=True), masks, f"B={B}")
    runs = la.rle_encode(np.stack(masks))                                    # host masks -> pack_mask_bits -> encoder
    assert split(runs.counts, runs.offsets) == want_of(masks)
    import torch
    runs = la.rle_encode(torch.as_tensor(np.stack(masks), device="cuda"))    # device bool masks
    assert split(runs.counts, runs.offsets) == want_of(masks)


def test_golden_masks_give_the_reference_counts(la, golden):
    """every mask of g8_masks.npz: decoded by the oracle, packed, encoded on the GPU == the reference's own recorded counts"""
    g = golden("g8_masks.npz")
    offs = np.concatenate([[0], np.cumsum(g["lens"])])
    recorded = [g["counts"][offs[i]:offs[i + 1]].tolist() for i in range(len(g["lens"]))]
    H, W = g["masks"].shape[1:]
    masks = np.stack([O.rle_decode(c, H, W) for c in recorded])
    runs = la.rle_encode_bits(la.pack_mask_bits(masks))
    assert split(runs.counts, runs.offsets) == recorded
    np.testing.assert_array_equal(np_(runs.offsets), offs)
    objs = la.rle_objects(runs, compress=True)
    assert [o["size"] for o in objs] == [[H, W]] * len(recorded)
    assert [la.rle_from_string(o["counts"]).tolist() for o in objs] == recorded
    assert [o["counts"].encode() for o in objs] == [O.rle_to_string(c) for c in recorded]
    assert la.rle_objects(runs) == [{"size": [H, W], "counts": c} for c in recorded]


# ------------------------------------------------------------------------------------------
# 2. the protocol of the two C calls
# ------------------------------------------------------------------------------------------
def c_block(la, mb, B):
    import torch
    from labelany3d_amd import _lib

    dev = mb.bits.device
    t = dict(runs=torch.full((B,), -7, dtype=torch.int32, device=dev), offsets=torch.full((B + 1,), -7, dtype=torch.int64, device=dev),
             status=torch.full((B,), -7, dtype=torch.int32, device=dev),
             ws=torch.zeros(max(int(_lib.lib.la3d_rle_encode_workspace_bytes(B, mb.H, mb.W)) // 8, 1), dtype=torch.int64, device=dev))
    a = _lib.RleEncodeArgs(struct_size=C.sizeof(_lib.RleEncodeArgs), B=B, H=mb.H, W=mb.W, frame_width=0 if mb.frame_width == mb.W else mb.frame_width,
                           mask_bits=mb.bits.data_ptr(), bits_plane_stride=int(mb.bits.stride(0)) if B > 1 else int(mb.bits.shape[1]),
                           runs=t["runs"].data_ptr(), offsets=t["offsets"].data_ptr(), status=t["status"].data_ptr(), workspace=t["ws"].data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
    return a, t


def c_stage(fn, a):
    from labelany3d_amd import _lib

    rc = getattr(_lib.lib, fn)(C.byref(a))
    assert rc == 0, (fn, rc, _lib.lib.la3d_last_error())


def test_capacity_one_short(la):
    import torch

    H, W = 37, 53
    masks = list(mask_set(H, W, seed=5).values())
    B, want = len(masks), want_of(masks)
    total = sum(len(w) for w in want)
    mb = mask_bits(la, masks, 64, garbage=True)
    a, t = c_block(la, mb, B)
    c_stage("la3d_rle_encode_offsets", a)
    counts = torch.full((total + 16,), SENTINEL, dtype=torch.int32, device="cuda")
    a.counts, a.capacity = counts.data_ptr(), total - 1
    c_stage("la3d_rle_encode", a)
    torch.cuda.synchronize()
    assert np_(t["runs"]).tolist() == [len(w) for w in want]
    offs = np_(t["offsets"])
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert np_(t["status"]).tolist() == [0] * (B - 1) + [1]                  # the last instance: LA3D_RLE_NO_ROOM
    got = np_(counts)
    assert (got[offs[B - 1]:] == SENTINEL).all()                             # nothing of it is written, nothing behind it
    assert split(got, offs)[:B - 1] == want[:B - 1]
    # the Python entry with the same capacity
    runs, status = la.rle_encode_bits(mb, capacity=total - 1, return_status=True)
    assert np_(status).tolist() == [0] * (B - 1) + [1] and split(runs.counts, runs.offsets)[:B - 1] == want[:B - 1]
    # room to spare: every instance exact, the tail untouched
    counts.fill_(SENTINEL)
    a.capacity = total + 16
    c_stage("la3d_rle_encode", a)
    torch.cuda.synchronize()
    assert np_(t["status"]).tolist() == [0] * B and split(np_(counts), offs) == want and (np_(counts)[total:] == SENTINEL).all()


def test_planes_changed_between_the_calls(la):
    import torch

    H, W = 37, 53
    rs = np.random.RandomState(9)
    masks = [rs.rand(H, W) < 0.3 for _ in range(4)]
    want = want_of(masks)
    offs = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    mb = mask_bits(la, masks, 64)
    a, t = c_block(la, mb, 4)
    c_stage("la3d_rle_encode_offsets", a)
    # instance 1 gets MORE runs than its range holds, instance 2 FEWER; 0 and 3 stay
    changed = [masks[0], rs.rand(H, W) < 0.5, np.zeros((H, W), bool), masks[3]]
    assert len(O.rle_encode(changed[1])["counts"]) > len(want[1])
    mb.bits.copy_(mask_bits(la, changed, 64).bits)
    counts = torch.full((int(offs[-1]) + 16,), SENTINEL, dtype=torch.int32, device="cuda")
    a.counts, a.capacity = counts.data_ptr(), int(offs[-1])
    c_stage("la3d_rle_encode", a)
    torch.cuda.synchronize()
    assert np_(t["status"]).tolist() == [0, 2, 2, 0]                         # LA3D_RLE_MISMATCH for the changed planes
    got = np_(counts)
    assert split(got, offs)[0] == want[0] and split(got, offs)[3] == want[3]   # the neighbours' ranges are theirs alone
    assert (got[offs[-1]:] == SENTINEL).all()                                # (what the changed planes left INSIDE their ranges means nothing)


def test_two_runs_are_bit_identical(la):
    H, W = 96, 160
    masks = list(mask_set(H, W, seed=11).values())
    mb = mask_bits(la, masks, 160)
    r1, r2 = la.rle_encode_bits(mb), la.rle_encode_bits(mb)
    assert np_(r1.counts).tobytes() == np_(r2.counts).tobytes() and np_(r1.offsets).tobytes() == np_(r2.offsets).tobytes()


def test_chain_with_capacity_is_capturable(la):
    """capacity given: no host synchronisation, so both stages are captured into a graph and replayed on other planes"""
    import torch

    H, W = 37, 53
    sets = [list(mask_set(H, W, seed=s).values()) for s in (21, 22)]
    wants = [want_of(s) for s in sets]
    cap = max(sum(len(w) for w in ws) for ws in wants) + 8
    mb = mask_bits(la, sets[0], 64)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        la.rle_encode_bits(mb, capacity=cap, stream=side)                    # (warm-up)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            runs, status = la.rle_encode_bits(mb, capacity=cap, stream=torch.cuda.current_stream(), return_status=True)
    for k in (1, 0):
        mb.bits.copy_(mask_bits(la, sets[k], 64).bits)
        runs.counts.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np_(status).tolist() == [0] * len(sets[k])
        assert split(runs.counts, runs.offsets) == wants[k]


# ------------------------------------------------------------------------------------------
# 3. round trips and consumers
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,pad", [(7, 33, True), (7, 33, False), (37, 53, True), (37, 53, False), (96, 160, True)])
def test_round_trips(la, H, W, pad):
    masks = np.stack(list(mask_set(H, W, seed=31).values()))
    mb = la.pack_mask_bits(masks, frame_pad=pad)
    runs = la.rle_encode_bits(mb)
    back = la.pack_rle_bits(runs, frame_pad=pad)
    nw = (H * mb.W + 31) // 32
    assert (back.H, back.W, back.frame_width) == (mb.H, mb.W, mb.frame_width)
    np.testing.assert_array_equal(np_(back.bits)[:, :nw], np_(mb.bits)[:, :nw])   # word for word
    np.testing.assert_array_equal(np_(la.rle_decode(runs)), masks)
    if (H, W) == (96, 160):
        np.testing.assert_array_equal(np_(la.mask_stats_rle(runs)), np_(la.mask_stats_bits(mb)))


@pytest.mark.parametrize("rgb", [False, True], ids=["u8", "rgb8"])
def test_label_maps_to_runs(la, rgb):
    rs = np.random.RandomState(41)
    H, W = 37, 53
    ids = [[3, 1, 9], [2, 200]]                                              # 9 is absent from image 0
    lab = np.stack([rs.choice([0, 1, 3, 5], (H, W)), rs.choice([0, 2, 200], (H, W))]).astype(np.uint8)
    assert not (lab[0] == 9).any()
    if rgb:
        big = [[3 + 256 * 7, 1 + 65536 * 2, 9], [2, 200 + 256 * 255]]
        maps = np.zeros((2, H, W, 3), np.uint8)
        for p in range(2):
            for small, full in zip(ids[p], big[p]):
                sel = lab[p] == small
                maps[p][sel] = [full & 255, (full >> 8) & 255, (full >> 16) & 255]
        lb = la.pack_label_bits(maps, big, rgb=True)
    else:
        lb = la.pack_label_bits(lab, ids)
    masks = [lab[p] == i for p in range(2) for i in ids[p]]
    runs = la.rle_encode_bits(lb.bits)
    assert split(runs.counts, runs.offsets) == want_of(masks)
    assert want_of(masks)[2] == [H * W]                                      # the absent id: one run of zeros


def test_fit_from_encoded_runs_equals_fit_from_masks(la):
    rs = np.random.RandomState(51)
    B, H, W = 8, 48, 64
    K = np.array([[50.0, 0, 32], [0, 50.0, 24], [0, 0, 1]])
    vv, uu = np.mgrid[0:H, 0:W]
    depth = (2.0 + 0.01 * uu + 0.02 * vv + 0.05 * rs.randn(B, H, W)).astype(np.float32)
    masks = np.zeros((B, H, W), bool)
    for i in range(B - 2):
        h, w = rs.randint(4, 40), rs.randint(4, 50)
        r0, c0 = rs.randint(0, H - h + 1), rs.randint(0, W - w + 1)
        masks[i, r0:r0 + h, c0:c0 + w] = True
    masks[B - 2] = rs.rand(H, W) < 0.05
    # masks[B - 1] stays empty
    runs = la.rle_encode(masks)
    b_r, s_r, _ = la.fit_instances_rle(depth, runs, K)
    b_m, s_m, _ = la.fit_instances(depth, masks, K)
    assert np_(s_r).tolist() == np_(s_m).tolist() and np_(s_m)[B - 1] != 0 and (np_(s_m)[:B - 2] == 0).all()
    got, ref = np_(b_r), np_(b_m)
    for i in range(B):
        if np_(s_m)[i]:
            assert np.isnan(got[i]).all()
            continue
        # (the tolerance of tests/test_gpu_masks.py::test_fit_from_rle_equals_fit_from_planes)
        np.testing.assert_allclose(got[i, :15], ref[i, :15], rtol=0, atol=1e-9 * max(1, np.abs(ref[i, :6]).max()))
        np.testing.assert_allclose(got[i, 15:], ref[i, 15:], rtol=0, atol=max(np.abs(ref[i, 15:]).max(), 1) * 2.0 ** -10)


# ------------------------------------------------------------------------------------------
# 4. the frames form: images of different sizes in one call
# ------------------------------------------------------------------------------------------
SIZES = [(8, 32), (37, 53), (96, 160)]
PER_IMAGE = [2, 3, 2]                                                        # seven instances


def frames_case(la):
    rs = np.random.RandomState(61)
    stacks, masks = [], []
    for (h, w), n in zip(SIZES, PER_IMAGE):
        ms = mask_set(h, w, seed=7)
        pick = [ms[k] for k in ("checker", "random0.5", "rectangle_corner")[:n]]
        stacks.append(np.stack(pick))
        masks += pick
    depth = [(2.0 + 0.01 * np.mgrid[0:h, 0:w][1] + 0.05 * rs.randn(h, w)).astype(np.float32) for h, w in SIZES]
    pf = la.pack_frames(depth)
    fb = la.pack_mask_bits_frames(la.pack_mask_frames(stacks))
    return pf, fb, masks


def test_frames_form_against_the_oracle(la):
    pf, fb, masks = frames_case(la)
    want = want_of(masks)
    (counts, offsets), sizes, status = la.rle_encode_bits_frames(pf, fb, return_status=True)
    assert np_(status).tolist() == [0] * 7
    assert split(counts, offsets) == want                                    # each instance on its own frame
    assert np_(sizes).tolist() == [list(m.shape) for m in masks]
    assert la.rle_objects((counts, offsets), sizes=sizes) == [{"size": list(m.shape), "counts": w} for m, w in zip(masks, want)]
    # the runs go back into planes, and into the fit
    img = np_(fb.image_index)
    back = la.pack_rle_bits_frames(pf, (counts, offsets), img)               # (host image_index: the layout of frame_bits_offsets)
    np.testing.assert_array_equal(np_(back.offsets), np_(fb.offsets))
    for n, o in enumerate(np_(fb.offsets)):
        nw = int(pf.table_host["H"][img[n]]) * int(pf.table_host["W"][img[n]]) // 32
        np.testing.assert_array_equal(np_(back.bits)[o:o + nw], np_(fb.bits)[o:o + nw], err_msg=f"plane {n}")
    K = np.array([[60.0, 0, 40], [0, 60.0, 30], [0, 0, 1]])
    from_runs = la.fit_instances_frames(pf, K, rles=(counts, offsets), image_index=fb.image_index)
    from_bits = la.fit_instances_frames_bits(pf, fb, K)
    assert np_(from_runs["status"]).tolist() == np_(from_bits["status"]).tolist()
    assert (np_(from_bits["status"]) == 0).any()


def test_frames_form_refuses_rows_on_the_device(la):
    import torch
    from labelany3d_amd import _lib

    pf, fb, masks = frames_case(la)
    want = want_of(masks)
    ii = np_(fb.image_index).copy()
    offs = np_(fb.offsets).copy()
    ii[2] = len(SIZES)                                                       # image_index = P
    offs[5] += 2                                                             # a plane offset that is no multiple of 4
    bad = fb._replace(image_index=torch.as_tensor(ii, device="cuda"), offsets=torch.as_tensor(offs, device="cuda"))
    keep = [n for n in range(7) if n not in (2, 5)]
    (counts, offsets), sizes, status = la.rle_encode_bits_frames(pf, bad, return_status=True)
    assert np_(status).tolist() == [5 if n in (2, 5) else 0 for n in range(7)]
    got = split(counts, offsets)
    assert got[2] == [] and got[5] == [] and [got[n] for n in keep] == [want[n] for n in keep]
    assert np_(sizes)[2].tolist() == [-1, -1]
    # through the C entries, into sentinel-filled counts: nothing is written for the refused rows, nothing behind the last range
    B, total = 7, sum(len(want[n]) for n in keep)
    t = dict(runs=torch.full((B,), -7, dtype=torch.int32, device="cuda"), offsets=torch.full((B + 1,), -7, dtype=torch.int64, device="cuda"),
             status=torch.full((B,), -7, dtype=torch.int32, device="cuda"), counts=torch.full((total + 16,), SENTINEL, dtype=torch.int32, device="cuda"),
             ws=torch.zeros(int(_lib.lib.la3d_rle_encode_workspace_bytes(B, pf.H, pf.W)) // 8, dtype=torch.int64, device="cuda"))
    a = _lib.RleEncodeArgs(struct_size=C.sizeof(_lib.RleEncodeArgs), B=B, H=pf.H, W=pf.W, P=len(SIZES), mask_bits=bad.bits.data_ptr(),
                           frames=pf.table.data_ptr(), image_index=bad.image_index.data_ptr(), bits_offsets=bad.offsets.data_ptr(),
                           runs=t["runs"].data_ptr(), offsets=t["offsets"].data_ptr(), counts=t["counts"].data_ptr(), status=t["status"].data_ptr(),
                           capacity=total + 16, workspace=t["ws"].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    c_stage("la3d_rle_encode_offsets", a)
    c_stage("la3d_rle_encode", a)
    torch.cuda.synchronize()
    assert np_(t["runs"]).tolist() == [0 if n in (2, 5) else len(want[n]) for n in range(7)]
    assert np_(t["status"]).tolist() == [5 if n in (2, 5) else 0 for n in range(7)]
    got = np_(t["counts"])
    assert (got[total:] == SENTINEL).all() and got[:total].tolist() == [c for n in keep for c in want[n]]
    # the shared case table (tests/frames_fault_rows.py), one fault per row, through the C entries: the table and the planes have pad
    # in front and behind, so a defect shows as a run too many or a wrong status, never as a fault.  (The entry takes no length.)
    fc = FR.case(end_check=False)
    rs = np.random.RandomState(5)
    ms = {n: rs.rand(*FR.GOOD[fc.rows[n][0]]) < 0.3 for n in fc.good}
    inbuf = FR.input_words(fc, rs, lambda n, h, w: plane_words(ms[n], FR.padded(w), garbage=True))
    d = FR.on_device(fc, inbuf)
    want = {n: O.rle_encode(ms[n])["counts"] for n in fc.good}
    B, total = fc.B, sum(len(w) for w in want.values())
    t = dict(runs=torch.full((B,), -7, dtype=torch.int32, device="cuda"), offsets=torch.full((B + 1,), -7, dtype=torch.int64, device="cuda"),
             status=torch.full((B,), -7, dtype=torch.int32, device="cuda"), counts=torch.full((total + 16,), SENTINEL, dtype=torch.int32, device="cuda"),
             ws=torch.zeros(int(_lib.lib.la3d_rle_encode_workspace_bytes(B, fc.H, fc.W)) // 8, dtype=torch.int64, device="cuda"))
    a = _lib.RleEncodeArgs(struct_size=C.sizeof(_lib.RleEncodeArgs), B=B, H=fc.H, W=fc.W, P=fc.P, mask_bits=d.bits.data_ptr(),
                           frames=d.table.data_ptr(), image_index=d.image_index.data_ptr(), bits_offsets=d.offsets.data_ptr(),
                           runs=t["runs"].data_ptr(), offsets=t["offsets"].data_ptr(), counts=t["counts"].data_ptr(), status=t["status"].data_ptr(),
                           capacity=total + 16, workspace=t["ws"].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    c_stage("la3d_rle_encode_offsets", a)
    c_stage("la3d_rle_encode", a)
    torch.cuda.synchronize()
    for n, (img, fault) in enumerate(fc.rows):
        assert (int(t["runs"][n]), int(t["status"][n])) == ((len(want[n]), 0) if fault is None else (0, 5)), (n, fault)
    got = np_(t["counts"])
    assert (got[total:] == SENTINEL).all() and got[:total].tolist() == [x for n in fc.good for x in want[n]]
    np.testing.assert_array_equal(np_(d.bits_all).view(np.uint32), inbuf)
    # every good row equals the call without the bad rows
    (counts, offsets), sizes, status = la.rle_encode_bits_frames(FR.frame_grid(la, fc, d), FR.frame_bits(la, fc, d, fc.good), return_status=True)
    assert np_(status).tolist() == [0] * len(fc.good) and split(counts, offsets) == [want[n] for n in fc.good]
    assert np_(sizes).tolist() == [list(ms[n].shape) for n in fc.good]
