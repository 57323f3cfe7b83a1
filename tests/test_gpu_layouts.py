"""GPU tests of the layout freedom the C-ABI gives a foreign caller (include/la3d.h, la3d_fit_args): plane strides other than H*W,
K records longer than 9 doubles, base pointers that are not 16-byte aligned, one shared plane given two ways, frame_width with
ground / subsample / the fused filter, and the host-pointer annotation entry with its own K sizing.  The Python wrappers always pass
stride H*W or 0, k_stride 9 or 0 and aligned buffers, so nothing else sends these layouts through the kernels.

Two kinds of check:
  * a layout that keeps the call on the same path (a plane stride H*W + 4k, a K record padded to 12 / 16 doubles) must give records,
    status and aux BIT-IDENTICAL to the contiguous call: same path, same arithmetic;
  * a layout that moves the call off the 16-byte vector path (stride H*W + 1 / + 3, a depth base one float past a 16-byte boundary,
    a u8 mask base 1 ... 15 bytes past one) is held to the CPU oracle: status, n_valid, n_masked exactly, the records by
    test_gpu_parity.assert_records with the reference_axis_noise rule.

GPU safety: every offset or strided view is carved from ONE device buffer allocated with the extra elements it needs, so no plane,
mask or K record reaches past its allocation, and no layout passed here lets a kernel read out of bounds.  These are correctness
tests, not fault probes."""
import ctypes as C

import numpy as np
import pytest

from oracle import la3d_oracle as O
from oracle.campaigns import engines as E

from .test_gpu_parity import assert_records, reference_axis_noise

pytestmark = pytest.mark.gpu

ENGINES = [None, "instance", "band", "rows", "rows2", "split"]
FRAMES = [(480, 640), (375, 500)]


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def _case(seed, B, H, W, P, polygons=False):
    """B instances on P planes (image_index when P != B): masks of the engine campaign's kinds (or its polygon annotations), its depth
    planes (invalid pixels included), per-plane K, a ground array with un-grounded and degenerate rows, subsample indices."""
    rs = np.random.RandomState(seed)
    depth = np.stack([E.one_plane(rs, H, W) for _ in range(P)])
    segs = None
    if polygons:
        ms = [E.one_polygon_mask(rs, H, W) for _ in range(B)]
        masks, segs = np.stack([m for m, _ in ms]), [s for _, s in ms]
    else:
        masks = np.stack([E.one_mask(rs, H, W) for _ in range(B)])
    masks[-1] = False                                            # one empty mask: status 1
    if polygons:
        segs[-1] = []                                            # (a segmentation without parts)
    ii = None if P == B else rs.randint(0, P, B).astype(np.int32)
    if ii is not None:
        ii[:P] = np.arange(P)                                    # every plane used
    K = np.stack([[[f, 0, W / 2 + rs.uniform(-20, 20)], [0, f * rs.uniform(0.9, 1.1), H / 2 + rs.uniform(-20, 20)], [0, 0, 1]]
                  for f in rs.uniform(0.6, 1.5, P) * W])
    ground = np.array([[0.05, -0.97, 0.1, 1.2]] * B) + 0.05 * rs.randn(B, 4)
    ground[1::3, 0] = np.nan                                     # "no ground" for these instances
    ground[2] = [0, -1, 0, 1.0]                                  # already aligned: the reference's degenerate case
    counts = masks.reshape(B, -1).sum(1)
    sidx = np.zeros((B, 500), np.int32)
    for n, c in enumerate(counts):
        if c > 500:
            sidx[n] = rs.randint(0, int(c), 500)
    return dict(depth=depth.astype(np.float32), masks=masks, segs=segs, K=K, ii=ii, ground=ground, sidx=sidx, B=B, H=H, W=W, P=P)


def _oracle(c, ground=None, sidx=None):
    """(records, status, n_valid, kappa) of the CPU oracle for a case, plane by plane."""
    masks, depth = c["masks"], c["depth"]
    g = None if ground is None else [None if np.isnan(r[0]) else r for r in ground]
    rec, st, nv, kap = (np.full((c["B"], 39), np.nan), np.zeros(c["B"], np.int32), np.zeros(c["B"], np.int64), np.full(c["B"], np.nan))
    di = np.arange(c["B"]) if c["ii"] is None else c["ii"]
    for p in range(c["P"]):   # (the oracle caches one plane at a time)
        sel = np.flatnonzero(di == p)
        if len(sel):
            r_, s_, _, n_, k_ = O.fit_instances(depth[p:p + 1], masks[sel], c["K"][p:p + 1], ground=None if g is None else [g[i] for i in sel],
                                                sample_idx=None if sidx is None else sidx[sel], depth_index=np.zeros(len(sel), np.int32),
                                                return_kappa=True)
            rec[sel], st[sel], nv[sel], kap[sel] = r_, s_, n_, k_
    return rec, st, nv, kap


_ORACLE = {}


def _oracle_cached(key, c, ground=None, sidx=None):
    if key not in _ORACLE:
        _ORACLE[key] = _oracle(c, ground, sidx)
    return _ORACLE[key]


class Dev:
    """Device buffers of one case, laid out as a foreign caller may lay them out, each carved from one allocation sized for the layout."""

    def __init__(self, la, c):
        import torch

        self.torch, self.la, self.c = torch, la, c
        self.dev = torch.device("cuda", 0)
        self.keep = []
        self.packed = {}

    def t(self, a, dt):
        x = self.torch.as_tensor(np.ascontiguousarray(a), device=self.dev).to(dt)
        self.keep.append(x)
        return x

    def ptr(self, x, byte_off=0):
        return None if x is None else C.c_void_p(x.data_ptr() + byte_off)

    def rle(self):
        """(counts, offsets) of the case's masks as run lengths, packed and uploaded once."""
        if "rle" not in self.packed:
            cnt, off, _, _ = self.la.pack_rle([O.rle_encode(m) for m in self.c["masks"]])
            self.packed["rle"] = (self.ptr(self.t(cnt, self.torch.int32)), self.ptr(self.t(off, self.torch.int64)))
        return self.packed["rle"]

    def poly(self):
        """(xy, ring_offsets, inst_rings) of the case's polygon annotations, packed and uploaded once."""
        if "poly" not in self.packed:
            xy, ro, ir, _, _ = self.la.pack_polygons(self.c["segs"], self.c["H"], self.c["W"])
            self.packed["poly"] = tuple(self.ptr(self.t(x, dt)) for x, dt in ((xy, self.torch.int32), (ro, self.torch.int64), (ir, self.torch.int64)))
        return self.packed["poly"]

    def depth(self, stride, base_off=0):
        """The case's planes (P,H,W) at element offset base_off + p * stride of one f32 buffer of base_off + (P-1)*stride + H*W
        elements (stride 0: the first plane only)."""
        d = self.c["depth"]
        HW = self.c["H"] * self.c["W"]
        n = base_off + (len(d) - 1) * stride + HW
        buf = self.torch.full((n,), float("nan"), dtype=self.torch.float32, device=self.dev)   # the gaps hold NaN: nothing reads them
        for p in range(len(d) if stride else 1):
            buf[base_off + p * stride:base_off + p * stride + HW] = self.torch.as_tensor(d[p].ravel(), device=self.dev)
        self.keep.append(buf)
        return self.ptr(buf, 4 * base_off)

    def mask(self, byte_off=0):
        """u8 planes (B,H*W) at byte offset byte_off of a buffer of byte_off + B*H*W bytes."""
        m = self.c["masks"].reshape(self.c["B"], -1).astype(np.uint8)
        buf = self.torch.zeros(byte_off + m.size, dtype=self.torch.uint8, device=self.dev)
        buf[byte_off:] = self.torch.as_tensor(m.ravel(), device=self.dev)
        self.keep.append(buf)
        return self.ptr(buf, byte_off)

    def K(self, k_stride, Ks=None):
        """K records of k_stride doubles (the padding NaN), one per plane; k_stride 0: the first matrix only."""
        Ks = self.c["K"] if Ks is None else Ks
        if k_stride == 0:
            return self.ptr(self.t(Ks[0].ravel(), self.torch.float64))
        rec = np.full((len(Ks), k_stride), np.nan)
        rec[:, :9] = Ks.reshape(len(Ks), 9)
        return self.ptr(self.t(rec.ravel(), self.torch.float64))


def _fit(la, d, *, depth, stride, K, k_stride, mask=None, kind="u8", image_index=None, ground=None, sidx=None, proj_size=None,
         engine=None, filt=None, area_hint=None, W=None, frame_width=0):
    """One la3d_fit_instances_ex call -> dict of NumPy arrays (boxes, status, aux, proj, stats)."""
    import torch

    from labelany3d_amd._lib import FitArgs, lib
    from labelany3d_amd.options import codes

    c = d.c
    B, H = c["B"], c["H"]
    W = c["W"] if W is None else W
    f = la.InstanceFitter(B, H, W, d.dev)
    f.boxes.fill_(-1.0); f.aux.fill_(-1.0); f.status.fill_(-1)
    proj = torch.full((B, 8), -1.0, dtype=torch.float64, device=d.dev)
    stats = torch.full((B, 4), -1, dtype=torch.int32, device=d.dev)
    p = d.ptr
    a = FitArgs(struct_size=C.sizeof(FitArgs), B=B, H=H, W=W, depth=depth, depth_plane_stride=stride, K=K, k_stride=k_stride,
                image_index=p(None if image_index is None else d.t(image_index, torch.int32)),
                ground=p(None if ground is None else d.t(ground, torch.float64)),
                sample_idx=p(None if sidx is None else d.t(sidx, torch.int32)),
                area_hint=p(None if area_hint is None else d.t(area_hint, torch.int32)),
                out=p(f.boxes[0]), status=p(f.status[0]), aux=p(f.aux[0]), workspace=p(f.workspace[0]),
                stream=C.c_void_p(torch.cuda.current_stream().cuda_stream), frame_width=frame_width)
    if kind == "u8":
        a.mask = mask
    elif kind == "rle":
        a.rle_counts, a.rle_offsets = d.rle()
    else:
        a.poly_xy, a.ring_offsets, a.inst_rings = d.poly()
    if filt is not None:
        a.filter_boundary, a.filter_min_area, a.filter_max_edge = filt
        a.stats = p(stats)
    if proj_size is not None:
        a.proj, a.image_width, a.image_height = p(proj), float(proj_size[0]), float(proj_size[1])
    a.opt_engine, a.opt_launch_order, a.opt_build = codes(engine=engine)
    rc = lib.la3d_fit_instances_ex(C.byref(a))
    assert rc == 0, lib.la3d_last_error().decode()
    torch.cuda.synchronize()
    return dict(boxes=f.boxes[0].cpu().numpy().copy(), status=f.status[0].cpu().numpy().copy(), aux=f.aux[0].cpu().numpy().copy(),
                proj=proj.cpu().numpy(), stats=stats.cpu().numpy())


def _same(x, y, what):
    for k in ("status", "boxes", "aux", "proj", "stats"):
        assert x[k].tobytes() == y[k].tobytes(), f"{what}: {k} differs"   # bit for bit, NaN records included


def _vs_oracle(c, got, ref, what, proj_size=None, keep=None):
    """status, n_valid, n_masked exactly; records by assert_records with the reference's own axis noise; the epilogue's 2-D boxes."""
    rec, st, nv, kap = ref
    if keep is not None:   # the fused filter: dropped instances carry status 6 and a NaN record
        st = np.where(keep, st, 6).astype(np.int32)
        rec = np.where(keep[:, None], rec, np.nan)
    b, s, aux = got["boxes"], got["status"], got["aux"]
    assert s.tolist() == st.tolist(), f"{what}: status"
    ok = st == 0
    assert (st != 0).any() and ok.any(), what                            # (a real batch: boxes fitted, instances rejected)
    assert np.isnan(b[~ok]).all(), f"{what}: a rejected record is not NaN"
    np.testing.assert_array_equal(aux[ok, 2], c["masks"].reshape(c["B"], -1).sum(1)[ok], err_msg=f"{what}: n_masked")
    np.testing.assert_array_equal(aux[ok, 1], nv[ok], err_msg=f"{what}: n_valid")
    chk = ok & (aux[:, 3] >= 1e-9)
    noise = reference_axis_noise(kap, aux[:, 1], aux[:, 3])
    assert_records(b[chk], rec[chk], what, gap=aux[chk, 3], noise=noise[chk])
    if proj_size is not None:
        Kp = c["K"][np.arange(c["B"]) if c["ii"] is None else c["ii"]]
        with np.errstate(invalid="ignore", divide="ignore"):
            want = O.project_boxes(b, Kp, proj_size)
        fin = ok & np.isfinite(want).all(1)
        np.testing.assert_allclose(got["proj"][fin], want[fin], rtol=1e-12, atol=1e-9, err_msg=f"{what}: 2-D boxes")
        assert np.isnan(got["proj"][~ok]).all(), f"{what}: 2-D boxes of a rejected instance are not NaN"


# ---------------------------------------------------------------------------------------------------------------------------------
# layouts that keep the path: bit-identical to the contiguous call
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "rle", "poly"])
@pytest.mark.parametrize("H,W", FRAMES)
def test_padded_plane_stride_is_bit_identical(la, H, W, kind):
    """depth_plane_stride = H*W + 4k (planes carved from one larger buffer) under every pinned engine, with and without ground."""
    c = _case(H + W + len(kind), B=12 if kind == "poly" else 24, H=H, W=W, P=12 if kind == "poly" else 24, polygons=kind == "poly")
    d = Dev(la, c)
    HW = H * W
    K = d.K(9)
    mask = d.mask() if kind == "u8" else None
    planes = {s: d.depth(s) for s in (HW, HW + 4, HW + 36)}
    for engine in ENGINES:
        for ground in (None, c["ground"]):
            kw = dict(K=K, k_stride=9, mask=mask, kind=kind, ground=ground, engine=engine, proj_size=(W, H))
            base = _fit(la, d, depth=planes[HW], stride=HW, **kw)
            assert (base["status"] == 0).any() and (base["status"] != 0).any()
            for s in (HW + 4, HW + 36):
                _same(_fit(la, d, depth=planes[s], stride=s, **kw), base, f"{kind} {H}x{W} stride HW+{s - HW} engine {engine} ground {ground is not None}")


@pytest.mark.parametrize("kind", ["u8", "rle", "poly"])
@pytest.mark.parametrize("H,W", FRAMES)
def test_padded_k_stride_is_bit_identical(la, H, W, kind):
    """k_stride 12 / 16 (per-plane K inside padded records, the padding NaN) with and without image_index, the projection on: the
    records, aux and 2-D boxes of k_stride 9.  And k_stride 0 (one shared K) against 9 with the matrix repeated."""
    for P, B in ((4, 16), (16, 16)):            # P planes + image_index, and private planes
        c = _case(H * 3 + P + len(kind), B=B, H=H, W=W, P=P, polygons=kind == "poly")
        d = Dev(la, c)
        dp = d.depth(H * W)
        mask = d.mask() if kind == "u8" else None
        Kr = np.repeat(c["K"][:1], P, 0)
        for engine in (None, "instance", "band", "split", "rows"):
            for ground in (None, c["ground"]):
                kw = dict(depth=dp, stride=H * W, mask=mask, kind=kind, image_index=c["ii"], ground=ground, engine=engine, proj_size=(W + 7, H - 5))
                base = _fit(la, d, K=d.K(9), k_stride=9, **kw)
                assert (base["status"] == 0).any()
                for ks in (12, 16):
                    _same(_fit(la, d, K=d.K(ks), k_stride=ks, **kw), base, f"{kind} {H}x{W} P={P} k_stride {ks} engine {engine}")
                _same(_fit(la, d, K=d.K(0), k_stride=0, **kw), _fit(la, d, K=d.K(9, Kr), k_stride=9, **kw),
                      f"{kind} {H}x{W} P={P} k_stride 0 vs repeated engine {engine}")


# ---------------------------------------------------------------------------------------------------------------------------------
# layouts that leave the vector path: against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
UNALIGNED = ["stride+1", "stride+3", "depth_base+1", "mask_base+1", "mask_base+7", "mask_base+15"]


@pytest.mark.parametrize("layout", UNALIGNED)
@pytest.mark.parametrize("H,W", FRAMES)
def test_unaligned_u8_layouts_vs_oracle(la, H, W, layout):
    """The scalar forms (launch_fit<false, ...>) on 640-wide frames, which otherwise take the single pass, the row, band and split
    engines: full-mask mode without ground, and ground + reference-subsample mode, the 2-D boxes of the epilogue on."""
    B = 12
    c = _case(7 * H, B=B, H=H, W=W, P=B)
    d = Dev(la, c)
    HW = H * W
    stride = HW + (1 if layout == "stride+1" else 3 if layout == "stride+3" else 0)
    dp = d.depth(stride, base_off=1 if layout == "depth_base+1" else 0)
    mask = d.mask(int(layout.split("+")[1]) if layout.startswith("mask_base") else 0)
    K = d.K(9)
    for ground, sidx in ((None, None), (c["ground"], c["sidx"])):
        ref = _oracle_cached((7 * H, H, W, ground is not None), c, ground, sidx)
        for engine in ENGINES:
            got = _fit(la, d, depth=dp, stride=stride, K=K, k_stride=9, mask=mask, ground=ground, sidx=sidx, engine=engine, proj_size=(W, H))
            _vs_oracle(c, got, ref, f"u8 {H}x{W} {layout} engine {engine} ground {ground is not None} sample {sidx is not None}", (W, H))


@pytest.mark.parametrize("kind", ["rle", "poly"])
@pytest.mark.parametrize("H,W", FRAMES)
def test_unaligned_depth_with_annotation_masks_vs_oracle(la, H, W, kind):
    """Run lengths / polygons: stride H*W + 1 / + 3 and a depth base one float past a 16-byte boundary against the oracle (ground,
    subsample mode, the projection).  (The u8 mask base does not enter the vector decision for them: la3d_fit_instances_ex takes
    exactly one of mask / rle_counts / poly_xy, so no u8 pointer travels with run lengths or polygons.)"""
    B = 10
    c = _case(11 * H + len(kind), B=B, H=H, W=W, P=B, polygons=kind == "poly")
    d = Dev(la, c)
    HW = H * W
    K = d.K(9)
    layouts = [(HW, 0), (HW + 1, 0), (HW, 1), (HW + 3, 1)]
    bufs = {lo: d.depth(lo[0], base_off=lo[1]) for lo in layouts}
    for ground, sidx in ((None, None), (c["ground"], c["sidx"])):
        ref = _oracle(c, ground, sidx)
        for engine in (None, "instance", "split"):
            kw = dict(K=K, k_stride=9, kind=kind, ground=ground, sidx=sidx, engine=engine, proj_size=(W, H))
            for stride, off in layouts:
                got = _fit(la, d, depth=bufs[stride, off], stride=stride, **kw)
                _vs_oracle(c, got, ref, f"{kind} {H}x{W} stride HW+{stride - HW} base+{off} engine {engine} ground {ground is not None}", (W, H))


# ---------------------------------------------------------------------------------------------------------------------------------
# one shared plane, two ways
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "rle"])
@pytest.mark.parametrize("H,W", FRAMES)
def test_shared_plane_stride0_vs_identical_planes(la, H, W, kind):
    """depth_plane_stride 0 against P identical planes with an image_index: both against the oracle; bit for bit under the engines
    whose choice does not depend on how the plane is addressed (the instance engine; the split engine for run lengths)."""
    B, P = 16, 4
    c = _case(13 * H + len(kind), B=B, H=H, W=W, P=P)
    c["depth"] = np.repeat(c["depth"][:1], P, 0)
    c["K"] = np.repeat(c["K"][:1], P, 0)
    d = Dev(la, c)
    K = d.K(0)
    mask = d.mask() if kind == "u8" else None
    shared, planes = d.depth(0), d.depth(H * W)
    for ground in (None, c["ground"]):
        ref = _oracle(c, ground)
        for engine in ENGINES:
            kw = dict(K=K, k_stride=0, mask=mask, kind=kind, ground=ground, engine=engine)
            g0 = _fit(la, d, depth=shared, stride=0, **kw)
            g1 = _fit(la, d, depth=planes, stride=H * W, image_index=c["ii"], **kw)
            for g, how in ((g0, "stride 0"), (g1, "identical planes")):
                _vs_oracle(c, g, ref, f"{kind} {H}x{W} {how} engine {engine} ground {ground is not None}")
            if engine == "instance":
                _same(g0, g1, f"{kind} {H}x{W} shared plane two ways, engine {engine}")


# ---------------------------------------------------------------------------------------------------------------------------------
# frame_width x ground x subsample x fused filter x pinned engine
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rle", "poly"])
def test_frame_width_with_ground_subsample_filter_engines(la, kind):
    """A 375 x 500 frame fitted as 375 x 512 with frame_width 500 (rows padded on the right), ground none / some / all, full-mask and
    subsample mode, the fused filter off and on, every pinned engine (the split engine falls back: its decoders know no padded rows)
    - against the oracle on the UNPADDED frame, and the filter's statistics / decisions against the oracle's."""
    H, Wf, Wp = 375, 500, 512
    B = 12
    c = _case(17 + len(kind), B=B, H=H, W=Wf, P=B, polygons=kind == "poly")
    padded = np.zeros((B, H, Wp), np.float32)
    padded[:, :, :Wf] = c["depth"]
    d = Dev(la, c)
    dp = d.ptr(d.t(padded.ravel(), d.torch.float32))
    K = d.K(9)
    g_all = c["ground"].copy()
    g_all[:, 0] = np.where(np.isnan(g_all[:, 0]), 0.05, g_all[:, 0])
    stats_ref = np.array([O.mask_stats(m, 3) for m in c["masks"]])
    keep = np.array([O.keep_instance(s, H, kind == "rle", 50) for s in stats_ref])
    for gname, ground in (("none", None), ("some", c["ground"]), ("all", g_all)):
        for sidx in (None, c["sidx"]):
            ref = _oracle(c, ground, sidx)
            for filt in (None, (3, 50, 10)):
                for engine in ENGINES:
                    what = f"{kind} frame_width {Wf} in {Wp} ground {gname} sample {sidx is not None} filter {filt} engine {engine}"
                    got = _fit(la, d, depth=dp, stride=H * Wp, K=K, k_stride=9, kind=kind, ground=ground, sidx=sidx, engine=engine,
                               filt=filt, W=Wp, frame_width=Wf)
                    if filt is not None:
                        np.testing.assert_array_equal(got["stats"], stats_ref, err_msg=what)
                        assert (~keep).any() and keep.any(), what
                    _vs_oracle(c, got, ref, what, keep=keep if filt is not None else None)


# ---------------------------------------------------------------------------------------------------------------------------------
# la3d_fit_annotations_host: its own plane count and K copy
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rle", "poly"])
def test_annotations_host_entry_k_stride_image_index_area_hint(la, kind):
    """The host-pointer entry with image_index, k_stride 12 and area_hint (la3d_points.hip sizes the plane count P and the K copy from
    them) gives what the device route gives, bit for bit: records, status, aux and the filter statistics."""
    import torch

    from labelany3d_amd._lib import FitArgs, lib

    H, W, B, P = 120, 160, 14, 3
    c = _case(23 + len(kind), B=B, H=H, W=W, P=P, polygons=kind == "poly")
    d = Dev(la, c)
    dp = d.depth(H * W)
    ks = 12
    Kh = np.full((P, ks), np.nan)
    Kh[:, :9] = c["K"].reshape(P, 9)
    hint = np.where(np.arange(B) % 2 == 0, c["masks"].reshape(B, -1).sum(1), 7).astype(np.int32)
    filt = (3, 50, 200)                                          # (keeps most of the campaign's masks, drops the smallest)
    dev = _fit(la, d, depth=dp, stride=H * W, K=d.K(ks), k_stride=ks, kind=kind, image_index=c["ii"], ground=c["ground"], filt=filt,
               area_hint=hint)
    # host arrays for every pointer but depth
    if kind == "rle":
        cnt, off, _, _ = la.pack_rle([O.rle_encode(m) for m in c["masks"]])
        host = dict(rle_counts=np.ascontiguousarray(cnt, np.int32), rle_offsets=np.ascontiguousarray(off, np.int64))
    else:
        xy, ro, ir, _, _ = la.pack_polygons(c["segs"], H, W)
        host = dict(poly_xy=np.ascontiguousarray(xy, np.int32), ring_offsets=np.ascontiguousarray(ro, np.int64),
                    inst_rings=np.ascontiguousarray(ir, np.int64))
    ii, gr, Kc = np.ascontiguousarray(c["ii"]), np.ascontiguousarray(c["ground"]), np.ascontiguousarray(Kh)
    out, aux = np.full((B, 39), -1.0), np.full((B, 4), -1.0)
    st, stats = np.full(B, -1, np.int32), np.full((B, 4), -1, np.int32)
    hp = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    a = FitArgs(struct_size=C.sizeof(FitArgs), B=B, H=H, W=W, depth=dp, depth_plane_stride=H * W, image_index=hp(ii), K=hp(Kc),
                k_stride=ks, ground=hp(gr), out=hp(out), status=hp(st), aux=hp(aux), stats=hp(stats), area_hint=hp(hint),
                stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for k, v in host.items():
        setattr(a, k, hp(v))
    a.filter_boundary, a.filter_min_area, a.filter_max_edge = filt
    assert lib.la3d_fit_annotations_host(C.byref(a)) == 0, lib.la3d_last_error().decode()
    assert (st == 0).any() and (st == 6).any() and (st != 0).any()
    _same(dict(boxes=out, status=st, aux=aux, proj=dev["proj"], stats=stats), dev, f"{kind} la3d_fit_annotations_host vs device route")
