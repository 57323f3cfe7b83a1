"""Batched, device-resident entry points over the C-ABI (include/la3d.h).

PyTorch is used only for device memory and streams; every computation is a HIP kernel in
libla3d.so.  Inputs may be torch tensors on the GPU (zero-copy) or NumPy arrays (uploaded).

The composition these functions implement is defined in SURVEY.md §3.3:
    boxes[n] = estimate_bbox(depth_to_points(depth[img(n)][None], K[img(n)])[masks[n]], None, ground[n], 'pca')
with depth_to_points = reference src/util.py:52-75 and estimate_bbox = reference
src/util_3dbox.py:106-178.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, options
from ._device import _as_dev, _bulk, _dev, _order, _ptr, _record, _stream, _upload_many  # noqa: F401  (_upload_many: passed on to old callers)
from ._lib import AUX, NSAMPLE, REC, FitArgs, check, lib


class Depth16(NamedTuple):
    """Depth planes stored in 16 bits (include/la3d.h "16-bit depth planes"; C-ABI ``la3d_fit_instances_depth16``), fitted where they
    lie - no float32 copy: ``data`` a resident (P,H,W) or (H,W) tensor of ``torch.float16`` (the value is float32(x), exact) or
    ``torch.uint16`` (the value is float32(x) * float32(scale), one rounding; with ``zero_is_hole`` a stored 0 is a hole - NaN -,
    dropped as a NaN depth is).  Planes may lie further apart than H*W elements (a slice of a larger tensor) and need only their
    element alignment.  ``frame_width``: the image columns when the rows are padded (what ``la3d_fit_args::frame_width`` says; 0 =
    all).  Accepted wherever ``fit_instances`` / ``fit_instances_ex`` / ``fit_instances_rle`` / ``fit_instances_poly`` /
    ``fit_instances_bits`` / ``InstanceFitter.run`` / ``run_bits`` take ``depth``; a plain float16 / uint16 array there is
    up-converted to float32 as before."""
    data: torch.Tensor
    scale: float = 1.0
    zero_is_hole: bool = True
    frame_width: int = 0


def _depth16_check(d16: Depth16, HW=None, frame: str = "masks") -> None:
    """The argument errors of a ``Depth16`` that need no device: dtype, scale, dimensions, the frame of the masks."""
    t = d16.data
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float16, torch.uint16):
        raise ValueError(f"Depth16 needs a torch.float16 or torch.uint16 tensor, not {getattr(t, 'dtype', type(t).__name__)}")
    if t.dtype == torch.uint16 and not (np.isfinite(np.float32(d16.scale)) and np.float32(d16.scale) > 0):
        raise ValueError(f"Depth16: scale must be finite and > 0 (as float32), not {d16.scale!r}")
    if t.dim() not in (2, 3):
        raise ValueError("Depth16 data must be (P,H,W) or (H,W)")
    if int(d16.frame_width) < 0 or int(d16.frame_width) > t.shape[-1]:
        raise ValueError("Depth16: frame_width must lie in [0, W]")
    if HW is not None and tuple(t.shape[-2:]) != tuple(HW):
        raise ValueError(f"depth planes {tuple(t.shape[-2:])} do not match {frame} {tuple(HW)}")


def _depth16_block(d16: Depth16, H: int, W: int) -> _lib.Depth16Block:
    """``la3d_depth16`` of a checked, resident ``Depth16`` whose planes are H x W: dense rows, planes >= H*W elements apart."""
    t = d16.data
    if not t.is_cuda:
        raise ValueError("Depth16 data must be resident on the GPU (it is fitted where it lies)")
    P = t.shape[0] if t.dim() == 3 else 1
    if (W > 1 and t.stride(-1) != 1) or (H > 1 and t.stride(-2) != W) or (t.dim() == 3 and P > 1 and t.stride(0) < H * W):
        raise ValueError(f"Depth16 planes must have dense rows and lie >= H*W elements apart (strides {t.stride()})")
    return _d16_block(t, d16.scale, d16.zero_is_hole, int(t.stride(0)) if t.dim() == 3 and P > 1 else 0)


def _d16_block(t: torch.Tensor, scale, zero_is_hole, plane_stride: int = 0) -> _lib.Depth16Block:
    """``la3d_depth16`` of resident float16 / uint16 words: planes ``plane_stride`` elements apart, or - 0 - one plane / the flat
    buffer of a ``PackedFrames16``.  Scale and hole rule count for uint16 only."""
    u16 = t.dtype == torch.uint16
    return _lib.Depth16Block(struct_size=C.sizeof(_lib.Depth16Block), dtype=_lib.DTYPE_U16 if u16 else _lib.DTYPE_F16,
                             planes=t.data_ptr(), plane_stride=plane_stride, scale=float(scale) if u16 else 1.0,
                             flags=_lib.DEPTH_ZERO_IS_HOLE if (u16 and zero_is_hole) else 0)


def refuse_depth16(depth, who: str) -> None:
    """The entries without a 16-bit form say so before any device work."""
    if isinstance(depth, Depth16):
        raise ValueError(f"{who} takes float32 depth planes only: Depth16 planes are fitted by fit_instances / fit_instances_ex / "
                         "fit_instances_rle / fit_instances_poly / fit_instances_bits / InstanceFitter.run (instance engine only)")


def _enqueue(a: FitArgs, bits=None, frames=None) -> None:
    """The C entry of a block built by ``_fit_args``, picked from what the call carries: a frame table (``frames`` = (pointer, P);
    with 16-bit depth - ``a.d16`` - its depth16 form; with ``bits`` = (pointer, offsets pointer, flags) its bit-plane form), 16-bit
    depth planes, bit planes (``bits`` = (pointer, stride, flags)), or the plain block."""
    d16 = getattr(a, "d16", None)
    if frames is not None:
        if bits is not None:
            check(lib.la3d_fit_instances_frames_bits(C.byref(a), None if d16 is None else C.byref(d16), frames[0], frames[1], bits[0], bits[1],
                                                     bits[2]), "la3d_fit_instances_frames_bits")
        elif d16 is not None:
            check(lib.la3d_fit_instances_frames_depth16(C.byref(a), C.byref(d16), frames[0], frames[1]), "la3d_fit_instances_frames_depth16")
        else:
            check(lib.la3d_fit_instances_frames(C.byref(a), frames[0], frames[1]), "la3d_fit_instances_frames")
    elif d16 is not None:
        b = bits if bits is not None else (None, 0, 0)
        check(lib.la3d_fit_instances_depth16(C.byref(a), C.byref(d16), b[0], b[1], b[2]), "la3d_fit_instances_depth16")
    elif bits is not None:
        check(lib.la3d_fit_instances_bits(C.byref(a), bits[0], bits[1], bits[2]), "la3d_fit_instances_bits")
    else:
        check(lib.la3d_fit_instances_ex(C.byref(a)), "la3d_fit_instances_ex")


def unpack_boxes(rec):
    """(B,39) record -> dict of center_cam (B,3), dimensions (B,3) = [dz,dy,dx], R_cam (B,3,3),
    bbox3D_cam (B,8,3): the four return values of the reference's estimate_bbox and the keys of its
    3dbbox.json (reference src/util_3dbox.py:283-290)."""
    return dict(center_cam=rec[..., 0:3], dimensions=rec[..., 3:6],
                R_cam=rec[..., 6:15].reshape(*rec.shape[:-1], 3, 3),
                bbox3D_cam=rec[..., 15:39].reshape(*rec.shape[:-1], 8, 3))


def mask_counts(masks, stream=None) -> torch.Tensor:
    """True pixels per mask plane (what the reference sees as in_pc.shape[0], :123)."""
    dev = masks.device if isinstance(masks, torch.Tensor) and masks.is_cuda else _dev()
    m = _as_dev(masks, torch.uint8, dev)
    B, H, W = m.shape
    out = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.la3d_mask_counts(_ptr(m), B, H, W, _ptr(out), _stream(stream)), "la3d_mask_counts")
    return out


def draw_sample_idx(counts, rng=None) -> np.ndarray:
    """The indices the reference would draw, in instance order, from the global NumPy stream:
    ``np.random.randint(0, N, 500)`` for every instance with N > 500 (reference
    src/util_3dbox.py:123-125); instances with N <= 500 consume nothing (row left 0)."""
    counts = np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts)
    rng = np.random if rng is None else rng
    idx = np.zeros((len(counts), NSAMPLE), np.int32)
    for n, c in enumerate(counts):
        if c > NSAMPLE:
            idx[n] = rng.randint(0, int(c), NSAMPLE)
    return idx


class InstanceFitter:
    """Reusable launch state for fit_instances on fixed (B,H,W): owns the output / status / aux /
    workspace buffers so the steady-state call allocates nothing and is a pure enqueue."""

    def __init__(self, B: int, H: int, W: int, device=None, slots: int = 1, ws_slots: int = 1, method: str = "pca"):
        """``method``: the yaw estimator the workspace is sized for ("convex_hull" needs the hand-off area of the hull finish,
        ``la3d_fit_workspace_bytes``) and the default of ``run``; a fitter sized for "convex_hull" also serves "pca" calls."""
        self.method = _lib.method_code(method)
        self.B, self.H, self.W = int(B), int(H), int(W)
        self.device = _dev(device)
        self.slots = slots
        nbytes = _lib.fit_workspace_bytes(self.B, self.H, self.W, self.method)
        wsz = max((nbytes + 255) // 256 * 256, 256)
        # ONE device allocation carved into the four buffers (a call through the convenience wrappers allocates once)
        up = lambda v: (v + 255) // 256 * 256  # noqa: E731  (every region starts 256-byte aligned, like a fresh allocation)
        nb, na, ns = slots * B * REC * 8, slots * B * AUX * 8, slots * B * 4
        o_aux, o_st, o_ws = up(nb), up(nb) + up(na), up(nb) + up(na) + up(ns)
        self._arena = torch.empty(o_ws + ws_slots * wsz, dtype=torch.uint8, device=self.device)
        self.boxes = self._arena[:nb].view(torch.float64).view(slots, B, REC)
        self.aux = self._arena[o_aux:o_aux + na].view(torch.float64).view(slots, B, AUX)
        self.status = self._arena[o_st:o_st + ns].view(torch.int32).view(slots, B)
        # one workspace per concurrently running call (calls on different streams must not share it)
        self.workspace = self._arena[o_ws:].view(ws_slots, wsz)

    def run(self, depth: torch.Tensor, masks: torch.Tensor, K: torch.Tensor, ground=None, sample_idx=None,
            image_index=None, slot: int = 0, stream=None, ws_slot: int = 0, engine=None, launch_order=None, build=None,
            area_hint=None, method=None):
        """All arguments already on the device with the ABI's dtypes (f32 / u8 / f64 / f64 / i32 / i32).
        ``depth``: float32 planes, or a ``Depth16`` (fitted from its 16-bit planes: C-ABI ``la3d_fit_instances_depth16``).
        ``engine`` / ``launch_order`` / ``build``: scheduling of THIS call (labelany3d_amd.options; speed only).
        ``method``: "pca" | "convex_hull" (None: what the fitter was built for)."""
        return self._run(self._method(method), depth, K, ground, sample_idx, image_index, slot, stream, ws_slot, (engine, launch_order, build),
                         area_hint, mask=_ptr(masks))

    def run_bits(self, depth: torch.Tensor, bits, K: torch.Tensor, ground=None, sample_idx=None, image_index=None, slot: int = 0,
                 stream=None, ws_slot: int = 0, engine=None, launch_order=None, build=None, area_hint=None, method=None,
                 frame_width: int = 0, height_rule: str = "rows"):
        """``run`` with the masks given as bit planes (C-ABI ``la3d_fit_instances_bits``; format: include/la3d.h "masks as bit
        planes"): ``bits`` is the tuple ``masks.pack_mask_bits`` returns, or an int32 device tensor (B, stride) whose rows hold the
        ``ceil(H*W/32)`` words of a plane stored ``self.W`` pixels wide (``frame_width``: the image columns when the rows are
        padded, 0 = all).  One launch (two for a hull call) on the caller's stream, capturable into a graph like ``run``."""
        meth = self._method(method)
        t, fw = (bits[0], bits[3]) if isinstance(bits, tuple) else (bits, int(frame_width))
        if isinstance(bits, tuple) and (bits[1], bits[2]) != (self.H, self.W):
            raise ValueError(f"bit planes of a {bits[1]} x {bits[2]} frame do not match the fitter's {self.H} x {self.W}")
        return self._run(meth, depth, K, ground, sample_idx, image_index, slot, stream, ws_slot, (engine, launch_order, build), area_hint,
                         bits=(_ptr(t), _bits_stride(t, self.B, self.H, self.W), height_rule), frame_width=0 if fw == self.W else fw)

    def _run(self, meth, depth, K, ground, sample_idx, image_index, slot, stream, ws_slot, sched, area_hint, mask=None, bits=None,
             frame_width=0):
        """The enqueue ``run`` and ``run_bits`` share - block, C entry, nothing else.  ``bits``: (pointer, stride, height rule)."""
        t = depth.data if isinstance(depth, Depth16) else depth   # (a Depth16 goes to _fit_args as it is, a tensor as its pointer)
        darg, planes = (depth if t is not depth else _ptr(t)), (t.shape[0] if t.dim() == 3 else 1)
        a = _fit_args(self.B, self.H, self.W, darg, planes, _ptr(K),
                      K.shape[0] if K.dim() == 3 else 1, _ptr(self.boxes[slot]), _ptr(self.status[slot]), _ptr(self.aux[slot]),
                      _ptr(self.workspace[ws_slot]), _stream(stream, raw=True), mask=mask, image_index=_ptr(image_index),
                      ground=_ptr(ground), sample_idx=_ptr(sample_idx), area_hint=_ptr(area_hint), opts=options.codes(*sched),
                      frame_width=frame_width, method=meth)
        _enqueue(a, bits and (bits[0], bits[1], height_rule_code(bits[2])))
        return self.boxes[slot], self.status[slot], self.aux[slot]

    def _method(self, method) -> int:
        """The LA3D_METHOD_* code of a call on this fitter; a hull call needs a fitter whose workspace was sized for it."""
        meth = self.method if method is None else _lib.method_code(method)
        if meth == _lib.METHOD_CONVEX_HULL and self.method != _lib.METHOD_CONVEX_HULL:
            raise ValueError("this InstanceFitter was sized for method='pca': build it with method='convex_hull'")
        return meth


def height_rule_code(height_rule) -> int:
    """``height_rule`` of the bit-plane entries -> LA3D_BITS_HEIGHT_*: "rows" = rows holding a pixel (the reference's rule for run-length
    annotations, src/util.py:368-369), "span" = last row - first row + 1 (polygons, :328-335)."""
    code = {"rows": _lib.BITS_HEIGHT_ROWS, "span": _lib.BITS_HEIGHT_SPAN}.get(height_rule) if isinstance(height_rule, str) else None
    if code is None:
        raise ValueError(f"unknown height_rule: {height_rule!r}. Use 'rows' or 'span'")
    return code


def _bits_stride(t, B: int, H: int, W: int) -> int:
    """The plane stride (words) of a bit-plane tensor, checked: int32 on the GPU, (B, >= ceil(H*W/32)), rows dense."""
    nwords = (H * W + 31) // 32
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.dim() == 2):
        raise ValueError("bit planes must be an int32 tensor (B, words) on the GPU")
    if t.shape[0] != B or t.shape[1] < nwords or (t.shape[1] > 1 and t.stride(1) != 1) or (B > 1 and t.stride(0) < nwords):
        raise ValueError(f"bit planes {tuple(t.shape)} (strides {t.stride()}) do not hold {B} planes of {nwords} words")
    return int(t.stride(0)) if B > 1 else max(int(t.shape[1]), nwords)


def _filter_args(filter):
    """``filter`` of fit_instances_rle / fit_instances_poly: True or a dict with the reference's three thresholds
    (src/util.py:291-326, :375): boundary strip width (10), minimum area (100), boundary pixels that make a mask "truncated" (10)."""
    f = {} if filter is True else dict(filter)
    unknown = set(f) - {"boundary_threshold", "scale_threshold", "truncation_pixels"}
    if unknown:
        raise ValueError(f"unknown filter keys: {sorted(unknown)}")
    b, a, e = int(f.get("boundary_threshold", 10)), int(f.get("scale_threshold", 100)), int(f.get("truncation_pixels", 10))
    if b < 0 or e <= 0:
        # the C-ABI reads filter_boundary < 0 or filter_max_edge <= 0 as "no filter" (a zero-initialised la3d_fit_args means none);
        # truncation_pixels <= 0 would mean "reject every instance" in the reference's rule (edge < 0 never holds): refuse it here
        # instead of silently fitting everything
        raise ValueError("filter: boundary_threshold must be >= 0 and truncation_pixels >= 1")
    return b, a, e


def _fit_args(B, H, W, depth, planes, K, nk, out, status, aux, workspace, stream, mask=None, rle=None, poly=None, image_index=None,
              ground=None, sample_idx=None, filter=None, stats=None, proj=None, image_size=None, area_hint=None, opts=(0, 0, 0),
              frame_width=0, method=0) -> FitArgs:
    """The argument block of every fit call (C-ABI ``la3d_fit_instances_ex``) from pointers (None = NULL; device pointers, or host
    pointers for ``la3d_fit_annotations_host``) and sizes: ``planes`` depth planes of H*W floats, ``nk`` intrinsics matrices (one
    of either is shared by every instance).  rle = (counts, offsets), poly = (xy, ring_offsets, inst_rings); ``filter`` as in
    ``fit_instances_rle`` (None: no filter); ``proj`` with ``image_size`` = (width, height); ``opts`` = options.codes().
    ``depth`` may be a ``Depth16``: the block then carries no depth (C-ABI ``la3d_fit_instances_depth16`` takes the planes beside
    it) and the ``la3d_depth16`` block rides along as ``a.d16`` - ``_enqueue`` picks the entry by it -, or that block itself, ready made
    (the flat buffer of a frames call).
    Built fresh for every call: one InstanceFitter may be driven from several threads and streams."""
    d16 = None
    if isinstance(depth, Depth16):
        _depth16_check(depth, (H, W), "the call's frame")
        d16, depth, planes = _depth16_block(depth, H, W), None, 1
    elif isinstance(depth, _lib.Depth16Block):
        d16, depth, planes = depth, None, 1
    a = FitArgs(struct_size=C.sizeof(FitArgs), B=B, H=H, W=W, depth=depth, depth_plane_stride=H * W if planes > 1 else 0,
                image_index=image_index, mask=mask, K=K, k_stride=9 if nk > 1 else 0, ground=ground, sample_idx=sample_idx,
                out=out, status=status, aux=aux, workspace=workspace, stream=stream, area_hint=area_hint, frame_width=frame_width,
                method=method)
    if rle is not None:
        a.rle_counts, a.rle_offsets = rle
    if poly is not None:
        a.poly_xy, a.ring_offsets, a.inst_rings = poly
    if filter:
        a.filter_boundary, a.filter_min_area, a.filter_max_edge = _filter_args(filter)
        a.stats = stats
    if image_size is not None:
        a.proj, a.image_width, a.image_height = proj, float(image_size[0]), float(image_size[1])
    a.opt_engine, a.opt_launch_order, a.opt_build = opts
    if d16 is not None:
        a.d16 = d16   # (a Python attribute beside the C fields: it keeps the block alive as long as ``a``)
    return a


def _check_image_index(given, ii, B, P):
    """image_index must lie in [0, P): an index outside makes the kernel read another allocation (the C-ABI takes no plane count).
    Host arrays are checked on the host, a device tensor on the device - on EVERY call: a tensor refilled through its data pointer
    (this library's kernels, another C-ABI user, a DLPack alias) keeps its object identity and its version counter, so no cache
    of "already checked" tensors is sound.  ~40 us (two reductions + the read-back) for a device tensor; `InstanceFitter.run` is
    the entry for callers that have validated their index once and loop."""
    if B == 0:
        return
    if not (isinstance(given, torch.Tensor) and given.is_cuda):
        h = np.asarray(given.numpy() if isinstance(given, torch.Tensor) else given)
        if h.min() < 0 or h.max() >= P:
            raise ValueError("image_index out of range")
        return
    lo, hi = torch.aminmax(ii)
    if int(lo) < 0 or int(hi) >= P:
        raise ValueError("image_index out of range")


def _fit_inputs(depth, K, image_index, ground, sample_idx, B, H, W, dev, frame, check_device_index=False, given_index=None, planes=None,
                expand_K=True, check_host_index=True):
    """The inputs every fit entry shares, checked against the call's B masks of H x W and on the device: depth (P,H,W) | (H,W)
    float32, K (P,3,3) | (3,3) float64 (a shared matrix is expanded to P), image_index (B,) int32, ground (B,4) float64,
    sample_idx (B,500) int32; None stays None.  ``frame`` names the masks in the error text.  The range of a host image_index is
    checked on the host (``given_index``: the array as the caller gave it, when it has been uploaded already); a device tensor's
    only with ``check_device_index`` (a ~40 us read-back).  Returns (depth, K, image_index, ground, sample_idx, P).
    A ``Depth16`` stays what it is - 16-bit planes where they lie, checked, ``data`` as (P,H,W) -; anything else becomes float32.
    ``planes``: the frames call - P comes from its frame table and ``depth`` (the flat buffer, checked by its wrapper) is passed through
    untouched.  That call differs in two more ways, kept as they are: ``expand_K=False`` - a shared K stays one matrix (``k_stride``
    0) instead of one per plane -, and ``check_host_index=False`` - the range of a host image_index is left to the device as well,
    where an index outside gives status 5 instead of an exception."""
    if planes is not None:
        d, dshape = depth, (planes, H, W)
    elif isinstance(depth, Depth16):
        _depth16_check(depth, (H, W), frame)
        if depth.data.is_cuda and depth.data.device != dev:
            raise ValueError("the Depth16 planes live on another device")
        d = depth._replace(data=depth.data if depth.data.dim() == 3 else depth.data[None])
        _depth16_block(d, H, W)   # (residency and strides, before anything is uploaded)
        dshape = d.data.shape
    else:
        d = _as_dev(depth, torch.float32, dev)
        if d.dim() == 2:
            d = d[None]
        dshape = d.shape
    if dshape[1:] != (H, W):
        raise ValueError(f"depth planes {tuple(dshape[1:])} do not match {frame} {(H, W)}")
    k = _as_dev(K, torch.float64, dev, cache=True)
    if k.dim() == 2:
        k = k[None]
    P = dshape[0]
    if k.shape[0] not in (1, P) or k.shape[1:] != (3, 3):
        raise ValueError("K must be (3,3) or (P,3,3)")
    if expand_K and k.shape[0] == 1 and P > 1:
        k = k.expand(P, 3, 3).contiguous()
    ii = None
    if image_index is not None:
        ii = _as_dev(image_index, torch.int32, dev)
        if ii.shape != (B,):
            raise ValueError("image_index must be (B,)")
        given = image_index if given_index is None else given_index
        if check_device_index or (check_host_index and not (isinstance(given, torch.Tensor) and given.is_cuda)):
            _check_image_index(given, ii, B, P)
    elif P not in (1, B):
        raise ValueError("without image_index, depth must have 1 or B planes")
    g = None
    if ground is not None:
        g = _as_dev(ground, torch.float64, dev)
        if g.shape != (B, 4):
            raise ValueError("ground must be (B,4)")
    si = None
    if sample_idx is not None:
        si = _as_dev(sample_idx, torch.int32, dev)
        if si.shape != (B, NSAMPLE):
            raise ValueError("sample_idx must be (B,500)")
    return d, k, ii, g, si, P


def _pad_rows16(d: Depth16, Wp: int) -> Depth16:
    """A ``Depth16`` whose rows are padded on the right to Wp columns with zero words (outside every mask: never fitted); the
    image columns stay in ``frame_width``.  A copy, for the small odd-width batches ``fit_instances`` pads - callers that care keep
    their planes padded (``pack_depth16(frame_pad=True)``)."""
    t = d.data
    W = int(t.shape[-1])
    out = torch.zeros(t.shape[:-1] + (Wp,), dtype=torch.int16, device=t.device)   # (bit patterns: uint16 has few kernels)
    out[..., :W].copy_(t.view(torch.int16))
    return d._replace(data=out.view(t.dtype), frame_width=int(d.frame_width) or W)


def pad_rows_f32(d: torch.Tensor, Wp: int) -> torch.Tensor:
    """(..., H, W) float32 on the device -> (..., H, Wp) with zeros on the right (C-ABI ``la3d_pad_rows``, current stream)."""
    W = int(d.shape[-1])
    d = d.contiguous()
    with torch.cuda.device(d.device):
        out = torch.empty(d.shape[:-1] + (Wp,), dtype=torch.float32, device=d.device)
        check(lib.la3d_pad_rows(_ptr(d), d.numel() // W, W, Wp, _ptr(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "la3d_pad_rows")
    return out


def padded_width(W: int) -> int:
    """The row length the tiled / single-pass forms of the fit want: the next multiple of 32."""
    return (int(W) + 31) // 32 * 32


def pad_depth_rows(depth, device=None):
    """Depth plane(s) (..., H, W) -> ((..., H, padded_width(W)) float32 on the device, W): rows padded on the right with zeros.
    COCO frames come in widths like 427, 500, 375, 333; with run-length / polygon masks such a frame is fitted as a frame of the
    padded width whose first W columns are image (C-ABI ``la3d_fit_args::frame_width``): 4-5 x faster than the row-linear form
    that odd widths otherwise take (profiles/r05/r05_frame_sizes.txt).  ``fit_instances_ex`` / ``fit_instances_rle`` /
    ``fit_instances_poly`` / ``fit_annotations*`` do this themselves; a caller that fits the same planes many times pads once and
    passes ``frame_width=W``."""
    dev = _dev(device)
    d = _as_dev(depth, torch.float32, dev)
    W = int(d.shape[-1])
    Wp = padded_width(W)
    if Wp == W:
        return d, W
    return pad_rows_f32(d, Wp), W


def fit_instances(depth, masks, K, ground=None, sample_idx=None, image_index=None, stream=None, device=None, method: str = "pca"):
    """Batched composed hot path on the GPU.

    depth        (P,H,W) or (H,W) float32 — P planes; one plane = shared by all instances
    masks        (B,H,W) bool / uint8 (non-zero = True), reference layout src/util.py:367,382
    K            (P,3,3) or (3,3) float64 pixel intrinsics
    ground       (B,4) float64 or None; rows whose first entry is NaN mean "no ground"
    sample_idx   None = full-mask mode; (B,500) int = reference-subsample mode (see draw_sample_idx)
    image_index  (B,) int — depth plane / K of each instance (default: instance n -> plane n, or 0)
    method       "pca" | "convex_hull": the reference's estimate_bbox argument (src/util_3dbox.py:146-151).  "convex_hull" = the
                 minimum-area rectangle over the hull edges of the footprint.  In full-mask mode it needs an instance without
                 ground rotation and a K without skew on a frame whose (padded) width is a multiple of 32; every other instance
                 comes back with status 5 (LA3D_BOX_UNSUPPORTED) and a NaN record - pass sample_idx there (every camera, every
                 ground).  aux[3] = -(hull vertices), or the eigen-gap (>= 0) where the reference's PCA fallback was taken.
    Returns (boxes (B,39) f64, status (B,) i32, aux (B,4) f64 = yaw, n_valid, n_masked, eigen-gap), on the GPU.
    """
    _lib.method_code(method)   # (the reference's error for an unknown method, before any device work)
    if isinstance(depth, Depth16):
        _depth16_check(depth, tuple(np.shape(masks))[-2:] if np.ndim(masks) == 3 else None)
    if device is None and isinstance(masks, torch.Tensor) and masks.is_cuda:
        device = masks.device
    dev = _dev(device)
    m = _as_dev(masks, torch.uint8, dev)
    if m.dim() != 3:
        raise ValueError("masks must be (B,H,W)")
    B, H, W = m.shape
    d, k, ii, g, si, P = _fit_inputs(depth, K, image_index, ground, sample_idx, B, H, W, dev, "masks", check_device_index=True)
    with torch.cuda.device(dev):
        hull = method == "convex_hull"   # (full-mask hull exists on the tiled path only: an odd width is padded at every batch size)
        if W % 32 != 0 and si is None and (2 <= B <= 256 or (hull and B >= 1)):
            # a small batch on a frame of odd width (COCO: 427, 500, 375, 333 ...): the tiled forms - and the row engine small batches
            # take - need word-aligned rows; padding the B mask planes and the depth rows with zeros costs less than the row-linear
            # form they would otherwise run (profiles/r05/r05_odd_width_u8.txt: 8 / 64 / 256 masks of 640x427: 172 / 198 / 202 us ->
            # 111 / 102 / 152 us per call).  Above 256 planes the copy costs what it saves: pad once yourself, or hand over annotations.
            Wp = (W + 31) // 32 * 32
            m = torch.nn.functional.pad(m, (0, Wp - W))
            if ii is not None and P > B:
                # a large resident stack of planes of which this call references at most B: pad the referenced planes only
                # (P = 1000 planes of 640x427 would otherwise be copied - 1 GB - on every call)
                sel = ii.long()
                d = d._replace(data=d.data.view(torch.int16).index_select(0, sel).view(d.data.dtype)) if isinstance(d, Depth16) else d.index_select(0, sel)
                if k.shape[0] > 1:
                    k = k.index_select(0, sel)
                ii, P = None, B
            d = _pad_rows16(d, Wp) if isinstance(d, Depth16) else pad_rows_f32(d, Wp)
            W = Wp
        f = InstanceFitter(B, H, W, dev, method=method)
        if B == 0:
            return f.boxes[0], f.status[0], f.aux[0]
        _order(stream)   # the arguments were uploaded / converted on the current stream
        out = f.run(d if (P > 1 or isinstance(d, Depth16)) else d[0], m, k, g, si, ii, stream=stream)
        _record(stream, d.data if isinstance(d, Depth16) else d, m, k, g, si, ii, f.workspace, f.boxes, f.status, f.aux)
        return out


def fit_points(clouds, ground=None, sample_idx=None, method: str = "pca", stream=None, device=None, small_clouds=None, _packed=False,
               hull_512=None):
    """estimate_bbox for a list of (N_i,3) clouds in one launch (reference src/util_3dbox.py:106-178).

    clouds: list of arrays/tensors, or a tuple (points (T,3) f64, offsets (B+1,) i64).
    small_clouds: True promises that no cloud has more than a few thousand rows to visit (LA3D_HINT_SMALL_CLOUDS: one wave per
    cloud); None = decided here when the cloud sizes are known on the host (a list of clouds, or sample_idx given).
    hull_512 (method="convex_hull"): True promises that no cloud holds more than 512 valid rows (LA3D_HINT_HULL_512: the kernel's
    small-LDS form, what the reference's 500-point clouds want); None = decided here from the cloud sizes when they are known on the
    host.  A cloud that breaks the promise comes back with status 5; without the promise the kernel holds 2048 rows per cloud.
    Returns (boxes (B,39), status (B,), aux (B,4)) on the GPU.
    """
    dev = _dev(device)
    hull512 = bool(hull_512)
    if isinstance(clouds, tuple):
        pts = _as_dev(clouds[0], torch.float64, dev)
        off = _as_dev(clouds[1], torch.int64, dev)
        if small_clouds is None:
            small_clouds = sample_idx is not None
    else:
        lens = [int(len(c)) for c in clouds]
        if hull_512 is None:
            hull512 = max(lens, default=0) <= 512      # (convex hull: the small-LDS form of the kernel, LA3D_HINT_HULL_512)
        if small_clouds is None:
            small_clouds = sample_idx is not None or max(lens, default=0) <= 4096
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        if not any(isinstance(c, torch.Tensor) for c in clouds):
            # host clouds (the reference's calling pattern): points, offsets and the other small host arguments in ONE copy
            hp = (np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds if len(c)]) if sum(lens)
                  else np.zeros((1, 3)))
            pts, off, ground, sample_idx = _bulk(dev, (hp, torch.float64), (offs, torch.int64), (ground, torch.float64), (sample_idx, torch.int32))
        else:
            off = torch.as_tensor(offs, device=dev)
            if sum(lens):
                pts = torch.cat([_as_dev(c, torch.float64, dev).reshape(-1, 3) for c in clouds if len(c)])
            else:
                pts = torch.zeros((1, 3), dtype=torch.float64, device=dev)
    B = off.numel() - 1
    meth = _lib.method_code(method)  # (reference :151)
    g = None if ground is None else _as_dev(ground, torch.float64, dev)
    si = None if sample_idx is None else _as_dev(sample_idx, torch.int32, dev)
    # one output buffer (records | aux | status): a caller that wants everything on the host reads it back in one copy
    packed = torch.empty(B * (REC + AUX) + (B + 1) // 2, dtype=torch.float64, device=dev)
    boxes = packed[:B * REC].view(B, REC)
    aux = packed[B * REC:B * (REC + AUX)].view(B, AUX)
    status = packed[B * (REC + AUX):].view(torch.int32)[:B]
    with torch.cuda.device(dev):
        check(lib.la3d_fit_points(_ptr(pts), _ptr(off), _ptr(g), _ptr(si), meth | (_lib.HINT_SMALL_CLOUDS if small_clouds else 0) | (_lib.HINT_HULL_512 if hull512 else 0), B, _ptr(boxes), _ptr(status),
                                  _ptr(aux), _stream(stream)), "la3d_fit_points")
    _record(stream, pts, off, g, si, packed)
    if _packed:
        return boxes, status, aux, packed
    return boxes, status, aux


def unproject(depth, K, R=None, t=None, out_dtype=torch.float64, stream=None, device=None) -> torch.Tensor:
    """depth (H,W) float32 -> (H,W,3) points on the GPU (reference src/util.py:52-75).  depth (P,H,W) with K (3,3) or (P,3,3):
    every frame in ONE launch -> (P,H,W,3) (``la3d_unproject_batch``; the reference's stage loops over the images)."""
    if device is None and isinstance(depth, torch.Tensor) and depth.is_cuda:
        device = depth.device
    dev = _dev(device)
    d = _as_dev(depth, torch.float32, dev)
    if d.dim() == 3:
        P, H, W = d.shape
        k = _as_dev(K, torch.float64, dev, cache=True).reshape(-1, 9)
        if k.shape[0] not in (1, P):
            raise ValueError("K must be (3,3) or (P,3,3)")
        Rt = None
        if R is not None or t is not None:
            Rt = (C.c_double * 12)(*(np.eye(3) if R is None else np.asarray(R, dtype=np.float64)).ravel(),
                                   *(np.zeros(3) if t is None else np.asarray(t, dtype=np.float64)).ravel())
        out = torch.empty((P, H, W, 3), dtype=out_dtype, device=dev)
        with torch.cuda.device(dev):
            check(lib.la3d_unproject_batch(_ptr(d), _ptr(k), 9 if k.shape[0] > 1 else 0, Rt, P, H, W, _ptr(out),
                                           int(out_dtype == torch.float64), _stream(stream)), "la3d_unproject_batch")
        _record(stream, d, k, out)
        return out
    H, W = d.shape
    K9 = (C.c_double * 9)(*np.asarray(K.cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64).ravel())
    Rt = None
    if R is not None or t is not None:
        Rm = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
        tv = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64)
        Rt = (C.c_double * 12)(*Rm.ravel(), *tv.ravel())
    out = torch.empty((H, W, 3), dtype=out_dtype, device=dev)
    with torch.cuda.device(dev):
        check(lib.la3d_unproject(_ptr(d), K9, Rt, H, W, _ptr(out), int(out_dtype == torch.float64), _stream(stream)),
              "la3d_unproject")
    return out
