"""Label maps and bit planes of images of different sizes in one call (include/la3d.h "images of different sizes in one call":
la3d_pack_label_bits_frames, la3d_fit_instances_frames_bits) on the GPU: the packer bit for bit against np.packbits, the fit against
the oracle image by image, against the run-length frames call of the same masks (the same engine on the same bit image), from
16-bit depth against the float32 call, the on-device refusals, and the whole chain captured into a graph.  The inputs
(tests/frames_bits_cases.py) are checked on the oracle alone by tests/test_frames_bits_contract.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import la3d_oracle as O

from . import frames_bits_cases as FC
from .test_gpu_bits import same_engine
from .test_gpu_frames import ground_rows, np_, oracle_mix
from .test_gpu_labels import DTYPES, ENDS, OUTSIDE, blocky, encode, palette
from .test_gpu_parity import assert_records

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
KEYS = ("boxes", "status", "aux")


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


_REF = {}


def case_and_ref(seed):
    """a case and the oracle's answer for it, computed once and shared (never written to)"""
    if seed not in _REF:
        case = FC.make_case(seed)
        _REF[seed] = (case, oracle_mix(case))
    return _REF[seed]


def trio(res):
    return tuple(np_(res[k]) for k in KEYS)


def check_fit(got, case, ref, tag, expect=None, sel=None):
    """status, n_in, n_valid equal; records by the eigen-gap rule of tests/test_gpu_parity.py at rtol = atol = 1e-9"""
    rec, st, yaw, nv = ref
    expect = st if expect is None else expect
    sel = np.arange(len(st)) if sel is None else sel
    boxes, status, aux = (np_(got[k])[sel] for k in KEYS)
    rec, nv, expect = rec[sel], nv[sel], expect[sel]
    np.testing.assert_array_equal(status, expect, err_msg=f"{tag} status")
    ok = expect == 0
    assert ok.any() and np.isnan(boxes[~ok]).all(), tag
    np.testing.assert_array_equal(aux[:, 2], [case["masks"][i].sum() for i in sel], err_msg=f"{tag} n_in")
    np.testing.assert_array_equal(aux[ok, 1], nv[ok], err_msg=f"{tag} n_valid")
    print(f"{tag}: {int(ok.sum())} of {len(ok)} fitted, max |record - oracle| {np.abs(boxes[ok] - rec[ok]).max():.3g}, smallest gap {aux[ok, 3].min():.3g}")
    assert_records(boxes[ok], rec[ok], tag, rtol=1e-9, gap=aux[ok, 3])


# ------------------------------------------------------------------------------------------
# 1. the packer, bit for bit
# ------------------------------------------------------------------------------------------
def packer_case(dtype, seed=7):
    """maps of eight cells whose ids hold the ends of the dtype (0 among them: real zeros next to the zero padding); per image all
    eight ids + the ids no map of the dtype can hold + a repeated id; one image without ids"""
    rs = np.random.RandomState(seed + len(dtype))
    pal = palette(rs, dtype, 8)
    assert set(ENDS[dtype]) <= set(pal.tolist()) and 0 in pal
    values = [pal[blocky(rs, h, w, 8, max(2, h // 6), max(4, w // 7))] for h, w in FC.SIZES]
    ids = [[] if p == FC.NO_IDS else [int(v) for v in pal] + list(OUTSIDE[dtype]) + [int(pal[1])] for p in range(len(FC.SIZES))]
    return values, ids


def rows_of(ids):
    img = np.repeat(np.arange(len(ids)), [len(x) for x in ids]).astype(np.int32)
    flat = np.concatenate([np.asarray(x, np.int64) for x in ids])
    return img, flat


def check_planes(fb, values, img, flat, offsets, tag, total):
    """every plane holds np.packbits of its mask on rows zero-padded to the pitch; every other word keeps the sentinel"""
    buf = np_(fb.bits).view(np.uint32)
    want = np.full(buf.shape, SENTINEL, np.uint32)
    areas = np.zeros(len(img), np.int64)
    for b, w in enumerate(FC.expected_words(values, img, flat)):
        want[offsets[b]:offsets[b] + len(w)] = w
        areas[b] = (values[img[b]] == flat[b]).sum()
    np.testing.assert_array_equal(np_(fb.offsets), offsets, err_msg=f"{tag} offsets")
    np.testing.assert_array_equal(buf[:total], want[:total], err_msg=f"{tag} words")
    assert (buf[total:] == SENTINEL).all(), f"{tag}: words behind the last plane were written"
    np.testing.assert_array_equal(np_(fb.area), areas, err_msg=f"{tag} area")
    np.testing.assert_array_equal(np_(fb.image_index), img, err_msg=f"{tag} image_index")


@pytest.mark.parametrize("dtype", DTYPES)
def test_packer_equals_packbits(la, dtype):
    import torch

    values, ids = packer_case(dtype)
    img, flat = rows_of(ids)
    pl = la.pack_label_frames([encode(v, dtype) for v in values], rgb=dtype == "rgb8")
    words = np.asarray([FC.SIZES[p][0] * FC.pitch(FC.SIZES[p][1]) // 32 for p in img], np.int64)
    assert {150, 14} <= set(words.tolist())
    # host ids: the planes follow each other, every start rounded up to 4 words
    step = (words + 3) // 4 * 4
    offsets = np.concatenate([[0], np.cumsum(step[:-1])])
    total = int(step.sum())
    assert (offsets % 4 == 0).all() and (step != words).any()       # some planes leave a gap: the sentinel must survive there
    out = torch.full((total + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    fb = la.pack_label_bits_frames(pl, ids, out=out)
    assert fb.bits.data_ptr() == out.data_ptr() and (fb.H, fb.W) == (pl.H, pl.W) == (120, 512)
    check_planes(fb, values, img, flat, offsets, f"{dtype} host ids", total)
    # zero asked of the padded frames: only image pixels answer
    zero_rows = [b for b in range(len(img)) if flat[b] == 0 and FC.SIZES[img[b]][1] % 32]
    assert zero_rows and all(np_(fb.area)[b] == (values[img[b]] == 0).sum() > 0 for b in zero_rows)
    # device ids: no synchronisation, the planes a uniform stride apart (the bounds' words rounded up to 4)
    lab = torch.as_tensor(flat.astype(np.int32), device="cuda")
    off = torch.as_tensor(np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.int32), device="cuda")
    stride = (pl.H * pl.W // 32 + 3) // 4 * 4
    out2 = torch.full((stride * len(img) + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    fb2 = la.pack_label_bits_frames(pl, (lab, off), out=out2)
    check_planes(fb2, values, img, flat, np.arange(len(img), dtype=np.int64) * stride, f"{dtype} device ids", stride * len(img))
    # without out=: the same words
    fb3 = la.pack_label_bits_frames(pl, ids)
    got = np_(fb3.bits).view(np.uint32)
    for b, w in enumerate(FC.expected_words(values, img, flat)):
        np.testing.assert_array_equal(got[offsets[b]:offsets[b] + len(w)], w)


@pytest.mark.parametrize("dtype", ["u8", "u16", "rgb8"])
def test_packer_reads_planes_at_any_conforming_offset(la, dtype):
    """depth_offset % 4 == 0 is all the contract asks: U8 / U16 planes that are not 16-byte aligned give the same words (4-byte loads),
    and what lies in the padding COLUMNS does not reach the planes"""
    import torch

    from labelany3d_amd.masks import FRAME_DTYPE

    values, ids = packer_case(dtype, seed=11)
    img, flat = rows_of(ids)
    c = 3 if dtype == "rgb8" else 1
    table = np.zeros(len(FC.SIZES), FRAME_DTYPE)
    off = 4
    for p, (h, w) in enumerate(FC.SIZES):
        table[p] = (off, h, FC.pitch(w), w, 0)
        off += h * FC.pitch(w) + 4 * (p % 3 + 1)            # gaps of 4, 8, 12 elements: offsets of every residue mod 16
    assert len({int(o) % 16 for o in table["depth_offset"]}) >= 3
    maps = [encode(v, dtype) for v in values]
    host = np.full((off + 16) * c, 0x33, maps[0].dtype)      # garbage between the planes and in the padding columns
    for m, row in zip(maps, table):
        o, h, wp, w = int(row["depth_offset"]), int(row["H"]), int(row["W"]), int(row["frame_width"])
        host[o * c:(o + h * wp) * c].reshape(h, wp * c)[:, :w * c] = m.reshape(h, w * c)
    data = torch.as_tensor(host.view(np.int16) if host.dtype == np.uint16 else host, device="cuda")
    tab = torch.as_tensor(np.ascontiguousarray(table).view(np.int32).reshape(-1, 6).copy(), device="cuda")
    code = {"u8": 0, "u16": 1, "rgb8": 3}[dtype]
    pl = la.PackedLabels(data, tab, table, 120, 512, list(FC.SIZES), code)
    fb = la.pack_label_bits_frames(pl, ids)
    got, offs = np_(fb.bits).view(np.uint32), np_(fb.offsets)
    for b, w in enumerate(FC.expected_words(values, img, flat)):
        np.testing.assert_array_equal(got[offs[b]:offs[b] + len(w)], w, err_msg=f"{dtype} row {b} (image {img[b]}, id {flat[b]})")


# ------------------------------------------------------------------------------------------
# 2. the fit against the oracle, image by image on the unpadded frames
# ------------------------------------------------------------------------------------------
def labels_call(la, case, pf=None, **kw):
    pf = la.pack_frames(case["depth"]) if pf is None else pf
    return la.fit_instances_frames_labels(pf, case["maps"], case["ids"], case["K"], **kw)


@pytest.mark.parametrize("seed", FC.SEEDS)
def test_fit_against_the_oracle(la, seed):
    import torch

    case, ref = case_and_ref(seed)
    np.testing.assert_array_equal(ref[1], case["expect"])        # (on the CPU, first)
    res = labels_call(la, case)
    fb = res["bits"]
    np.testing.assert_array_equal(np_(fb.image_index), case["img"])
    np.testing.assert_array_equal(np_(fb.area), [m.sum() for m in case["masks"]])
    check_fit(res, case, ref, f"seed {seed}")
    assert set(np_(res["status"]).tolist()) == {0, 1, 3}
    # the same planes in a shuffled order (image_index no longer sorted): every record follows its instance
    order = np.random.RandomState(seed + 3).permutation(len(case["img"]))
    t = torch.as_tensor(order, device="cuda")
    pf = la.pack_frames(case["depth"])
    got = la.fit_instances_frames_bits(pf, fb._replace(offsets=fb.offsets[t].contiguous(), image_index=fb.image_index[t].contiguous(),
                                                       area=fb.area[t].contiguous()), case["K"], area_hint=fb.area[t].contiguous())
    for k in KEYS:
        np.testing.assert_array_equal(np_(got[k]), np_(res[k])[order], err_msg=f"shuffled {k}")


@pytest.mark.parametrize("variant", ["ground", "sample", "proj"])
def test_fit_variants_against_the_oracle(la, variant):
    case, plain = case_and_ref(0)
    B = len(case["img"])
    if variant == "ground":
        g = ground_rows(B, 5)
        check_fit(labels_call(la, case, ground=g), case, oracle_mix(case, ground=g), "ground")
    elif variant == "sample":
        areas = np.asarray([m.sum() for m in case["masks"]])
        assert (areas > 500).sum() >= 8 and (areas <= 500).sum() >= 8        # both sides of the reference's subsample rule
        sidx = la.draw_sample_idx(areas, np.random.RandomState(9))
        ref = oracle_mix(case, sidx=sidx)
        np.testing.assert_array_equal(ref[1], case["expect"])
        check_fit(labels_call(la, case, sample_idx=sidx), case, ref, "subsample")
    else:
        res = labels_call(la, case, proj=True)
        check_fit(res, case, plain, "proj")
        rec, st = plain[0], plain[1]
        ok = st == 0
        size = [case["sizes"][p] for p in case["img"]]
        want = np.stack([O.project_boxes(rec[i:i + 1], case["K"][case["img"][i]], (size[i][1], size[i][0]))[0] for i in range(B)])
        got = np_(res["boxes2d"])
        np.testing.assert_allclose(got[ok], want[ok], rtol=1e-9, atol=1e-9, err_msg="2-D boxes")
        assert np.isnan(got[~ok]).all()
        # clamped to each instance's OWN frame, not to the bounds of the call
        assert (got[ok, 6] <= [s[1] for s, o in zip(size, ok) if o]).all() and (got[ok, 7] <= [s[0] for s, o in zip(size, ok) if o]).all()


# (blocky cells touch the border of frames this small all the time: a rule with the reference's 10 truncation pixels keeps nothing)
FILTER = {"boundary_threshold": 2, "scale_threshold": 60, "truncation_pixels": 120}


def keep_rule(stats, image_height, rows):
    """the keep rule of include/la3d.h ("instance filter fused into the fit") on the oracle's statistics: what O.keep_instance states
    with the reference's fixed 10 truncation pixels, here with the call's"""
    area, nrows, span, edge = stats
    return ((nrows if rows else span) / image_height > 0.0625) and edge < FILTER["truncation_pixels"] and area >= FILTER["scale_threshold"]


@pytest.mark.parametrize("rule", ["rows", "span"])
def test_fused_filter_both_height_rules(la, rule):
    case, ref = case_and_ref(1)
    stats = np.array([O.mask_stats(m, FILTER["boundary_threshold"]) for m in case["masks"]])
    keep = np.array([keep_rule(s, case["sizes"][p][0], rule == "rows") for s, p in zip(stats, case["img"])])
    assert keep.any() and (~keep).any(), "the inputs should exercise both sides of the keep rule"
    res = labels_call(la, case, filter=FILTER, height_rule=rule)
    np.testing.assert_array_equal(np_(res["stats"]), stats, err_msg="filter statistics")
    check_fit(res, case, ref, f"filter {rule}", expect=np.where(keep, ref[1], 6).astype(np.int32))


# ------------------------------------------------------------------------------------------
# 3. against fit_instances_frames with run lengths of the same masks: the same engine on the same bit image
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "ground+proj", "sample", "filter"])
def test_equals_the_run_length_frames_call(la, mode):
    case, _ = case_and_ref(2)
    B = len(case["img"])
    kw = {}
    if mode == "ground+proj":
        kw = dict(ground=ground_rows(B, 8), proj=True)
    elif mode == "sample":
        kw = dict(sample_idx=la.draw_sample_idx(np.asarray([m.sum() for m in case["masks"]]), np.random.RandomState(4)))
    elif mode == "filter":
        kw = dict(filter=FILTER)
    pf = la.pack_frames(case["depth"])
    got = labels_call(la, case, pf=pf, **kw)
    rle = la.fit_instances_frames(pf, case["K"], rles=[O.rle_encode(m) for m in case["masks"]], image_index=case["img"], **kw)
    same_engine(trio(got), trio(rle), mode)
    for k in ("stats", "boxes2d"):
        if k in rle:
            np.testing.assert_allclose(np.nan_to_num(np_(got[k]), nan=-7.0), np.nan_to_num(np_(rle[k]), nan=-7.0), rtol=1e-12, atol=1e-12, err_msg=k)


# ------------------------------------------------------------------------------------------
# 4. 16-bit depth: the float32 call on the up-converted planes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "u16"])
@pytest.mark.parametrize("sample", [False, True], ids=["full", "subsample"])
def test_16_bit_depth_equals_the_float32_call(la, dtype, sample):
    case, _ = case_and_ref(1)
    if dtype == "f16":
        stored = [d.astype(np.float16) for d in case["depth"]]
        up = [s.astype(np.float32) for s in stored]
        pf16 = la.pack_frames(stored, dtype="f16")
    else:
        scale = np.float32(0.001)
        stored = [np.rint(d / scale).astype(np.uint16) for d in case["depth"]]
        for s in stored:
            s[::5, ::7] = 0                                          # holes under the masks
        up = [np.where(s == 0, np.float32(np.nan), s.astype(np.float32) * scale).astype(np.float32) for s in stored]
        pf16 = la.pack_frames(stored, dtype="u16", scale=0.001, zero_is_hole=True)
    kw = dict(sample_idx=la.draw_sample_idx(np.asarray([m.sum() for m in case["masks"]]), np.random.RandomState(2))) if sample else {}
    got = labels_call(la, case, pf=pf16, proj=True, **kw)
    ref = labels_call(la, case, pf=la.pack_frames(up), proj=True, **kw)
    same_engine(trio(got), trio(ref), f"{dtype} {'subsample' if sample else 'full'}")
    np.testing.assert_array_equal(np.nan_to_num(np_(got["boxes2d"]), nan=-7.0), np.nan_to_num(np_(ref["boxes2d"]), nan=-7.0))
    assert (np_(got["status"]) == 0).sum() >= 28


# ------------------------------------------------------------------------------------------
# 5. on-device refusals
# ------------------------------------------------------------------------------------------
def test_refused_instances_get_status_5_and_nothing_is_written_for_them(la):
    import torch

    from labelany3d_amd import _lib

    case, ref = case_and_ref(0)
    img, B = case["img"], len(case["img"])
    flat = np.concatenate([np.asarray(x, np.int64) for x in case["ids"]])
    pf = la.pack_frames(case["depth"])
    pl = la.pack_label_frames(case["maps"])
    # a broken frame row, in the table the packer reads and in the one the fit reads: image 4 gets a pitch that is no multiple of 32
    BROKEN = 4
    for tab in (pf.table, pl.table):
        tab[BROKEN, 3] = 333
    offs_h, total = la.frame_bits_offsets(pl.table_host, img)
    rows4 = np.flatnonzero(img == BROKEN)
    two, neg, outside = int(np.flatnonzero(img == 0)[1]), int(np.flatnonzero(img == 6)[2]), int(np.flatnonzero(img == 5)[0])
    offs_bad = offs_h.copy()
    offs_bad[two], offs_bad[neg] = 2, -8
    ii_bad = img.copy()
    ii_bad[outside] = 99
    refused = np.zeros(B, bool)
    refused[rows4] = refused[[two, neg, outside]] = True
    assert refused.sum() == len(rows4) + 3 and (case["expect"][refused] == 0).all()
    # the planes sit 4096 words inside a larger allocation, so that a write through the negative offset would land in the sentinel
    MARGIN = 4096
    whole = torch.full((MARGIN + total + MARGIN,), SENTINEL, dtype=torch.int32, device="cuda")
    bits = whole[MARGIN:]
    lab = torch.as_tensor(flat.astype(np.int32), device="cuda")
    off = torch.as_tensor(np.concatenate([[0], np.cumsum([len(x) for x in case["ids"]])]).astype(np.int32), device="cuda")
    offs = torch.as_tensor(offs_bad, device="cuda")
    area = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    rc = _lib.lib.la3d_pack_label_bits_frames(C.c_void_p(pl.data.data_ptr()), pl.code, C.c_void_p(pl.table.data_ptr()), len(FC.SIZES), pl.H, pl.W,
                                              C.c_void_p(off.data_ptr()), C.c_void_p(lab.data_ptr()), B, C.c_void_p(bits.data_ptr()),
                                              C.c_void_p(offs.data_ptr()), C.c_void_p(area.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib.la3d_last_error()
    torch.cuda.synchronize()
    want = np.full(whole.numel(), SENTINEL, np.uint32)
    want_area = np.zeros(B, np.int64)
    packer_skips = refused.copy()
    packer_skips[outside] = False                                    # (the packer goes by inst_offsets: this row's plane IS written)
    for b, w in enumerate(FC.expected_words(case["values"], img, flat)):
        if not packer_skips[b]:
            want[MARGIN + offs_h[b]:MARGIN + offs_h[b] + len(w)] = w
            want_area[b] = case["masks"][b].sum()
    np.testing.assert_array_equal(np_(whole).view(np.uint32), want, err_msg="the packer wrote for a refused row (or missed a conforming one)")
    np.testing.assert_array_equal(np_(area), want_area)
    fb = la.FrameBits(bits, offs, torch.as_tensor(ii_bad, device="cuda"), area, pl.table_host, pl.H, pl.W)
    res = la.fit_instances_frames_bits(pf, fb, case["K"], proj=True)
    boxes, status, aux = trio(res)
    np.testing.assert_array_equal(status[refused], 5)
    assert np.isnan(boxes[refused]).all() and np.isnan(np_(res["boxes2d"])[refused]).all()
    assert np.isnan(aux[refused][:, [0, 2, 3]]).all() and (aux[refused, 1] == 0).all()
    check_fit(res, case, ref, "the others", sel=np.flatnonzero(~refused))


# ------------------------------------------------------------------------------------------
# 6. the whole chain captured into a graph
# ------------------------------------------------------------------------------------------
def test_labels_call_captured_into_a_graph(la):
    """resident depth, labels, ids and K: pack + fit are a chain on one stream, captured once and replayed with the labels changed
    in place; the second replay of each set matches an eager call"""
    import torch

    dev = torch.device("cuda", 0)
    case0 = FC.make_case(0)
    pf = la.pack_frames(case0["depth"])
    pl = la.pack_label_frames(case0["maps"])
    K = torch.as_tensor(case0["K"], device=dev)
    flat = np.concatenate([np.asarray(x, np.int64) for x in case0["ids"]]).astype(np.int32)
    lab = torch.as_tensor(flat, device=dev)
    off = torch.as_tensor(np.concatenate([[0], np.cumsum([len(x) for x in case0["ids"]])]).astype(np.int32), device=dev)
    side = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        la.fit_instances_frames_labels(pf, pl, (lab, off), K, stream=side)      # (warm-up: every small upload is cached)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            res = la.fit_instances_frames_labels(pf, pl, (lab, off), K, stream=torch.cuda.current_stream())
    for seed in (1, 2):
        case = FC.make_case(seed)
        assert case["ids"] == case0["ids"]
        pl.data.copy_(la.pack_label_frames(case["maps"]).data)                   # the labels change in place
        for replay in range(2):
            g.replay()
        torch.cuda.synchronize()
        got = trio(res)
        eager = la.fit_instances_frames_labels(pf, la.pack_label_frames(case["maps"]), case["ids"], K)
        for a, b, k in zip(got, trio(eager), KEYS):
            np.testing.assert_array_equal(a, b, err_msg=f"seed {seed} {k}")
        np.testing.assert_array_equal(np_(res["bits"].area), [m.sum() for m in case["masks"]])
