"""The torch plumbing every wrapper shares (device, uploads, pointers, the launch stream) and ``_int_arg``.  Imports ``_lib`` only."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib


def _dev(device=None) -> torch.device:
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise _lib.La3dError("no GPU visible: labelany3d_amd has no CPU path (libla3d.so is a HIP library)")
    return torch.device("cuda", torch.cuda.current_device())


_SMALL_UPLOADS: dict = {}   # (bytes, dtype, shape, device) -> device tensor: small host arrays that callers pass again and again (K)


def _as_dev(x, dtype, device, cache: bool = False) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x
        if t.dtype == torch.bool and dtype == torch.uint8:
            t = t.view(torch.uint8) if t.is_contiguous() else t.contiguous().view(torch.uint8)
        elif t.dtype != dtype:
            t = t.to(dtype)
        if t.device != device:
            t = t.to(device)
        return t.contiguous()
    a = np.asarray(x)
    if dtype == torch.uint8 and a.dtype == np.bool_:
        a = a.view(np.uint8)
    if cache and a.nbytes <= 1024:   # opt-in (the 3x3 intrinsics): one upload per distinct value instead of one per call
        key = (a.tobytes(), str(a.dtype), a.shape, dtype, str(device))
        hit = _SMALL_UPLOADS.get(key)
        if hit is None:
            if len(_SMALL_UPLOADS) > 256:
                _SMALL_UPLOADS.clear()
            t = torch.as_tensor(np.ascontiguousarray(a), device=device).to(dtype).contiguous()
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(device))       # the upload / conversion runs on the stream current NOW
            hit = _SMALL_UPLOADS[key] = (t, ev)
        t, ev = hit
        torch.cuda.current_stream(device).wait_event(ev)          # a later user on another stream is ordered behind the upload
        return t                                                  # read-only by contract: shared between callers
    return torch.as_tensor(np.ascontiguousarray(a), device=device).to(dtype).contiguous()


def _plane_source(x, dev, dtypes):
    """(B,H,W) input of a packer -> (tensor, plane stride in elements): a device tensor whose planes are dense (rows W apart, pixels
    adjacent) is read where it lies, whatever its plane stride and base alignment; everything else is made contiguous first."""
    if isinstance(x, torch.Tensor) and x.is_cuda and x.device == dev and x.dim() == 3 and x.dtype in dtypes:
        B, H, W = x.shape
        if (W == 1 or x.stride(2) == 1) and (H == 1 or x.stride(1) == W) and (B <= 1 or x.stride(0) >= H * W):
            t = x.view(torch.uint8) if x.dtype == torch.bool else x
            return t, (int(x.stride(0)) if B > 1 else H * W)
    t = _as_dev(x, dtypes[0] if not (isinstance(x, torch.Tensor) and x.dtype in dtypes) else x.dtype, dev)
    if t.dim() != 3:
        raise ValueError("expected (B,H,W)")
    return t, int(t.shape[1] * t.shape[2])


def _upload_many(arrays, device, pinned: Optional[torch.Tensor] = None):
    """Several small host arrays -> device tensors with ONE host-to-device copy (each separate upload costs ~17 us of launch
    overhead on this stack; the per-image wrappers have six to eight of them).  ``arrays``: list of (ndarray | None, torch dtype);
    None stays None.  The views share one device buffer (16-byte aligned pieces).  ``pinned``: a pinned uint8 staging buffer of at
    least the packed size - the copy is then asynchronous on the current stream (the caller keeps the buffer untouched until that
    stream has passed the copy)."""
    metas, total = [], 0
    for a, dt in arrays:
        if a is None:
            metas.append(None)
            continue
        h = np.ascontiguousarray(np.asarray(a))
        want = torch.empty(0, dtype=dt).numpy().dtype
        if h.dtype != want:
            h = h.astype(want)
        metas.append((h, total))
        total += (h.nbytes + 15) & ~15
    if total == 0:
        return [None if m is None else torch.empty(m[0].shape, dtype=arrays[i][1], device=device) for i, m in enumerate(metas)]
    if pinned is not None and pinned.numel() >= total:
        buf = pinned.numpy()[:total]
    else:
        pinned = None
        buf = np.empty(total, np.uint8)
    for m in metas:
        if m is not None and m[0].nbytes:
            buf[m[1]:m[1] + m[0].nbytes] = m[0].reshape(-1).view(np.uint8)
    if pinned is not None:
        dbuf = torch.empty(total, dtype=torch.uint8, device=device)
        dbuf.copy_(pinned[:total], non_blocking=True)
    else:
        dbuf = torch.as_tensor(buf, device=device)
    out = []
    for (a, dt), m in zip(arrays, metas):
        if m is None:
            out.append(None)
        else:
            h, off = m
            out.append(dbuf[off:off + h.nbytes].view(dt).view(h.shape))
    return out


def _bulk(device, *pairs):
    """(value, torch dtype) pairs -> the values with every HOST array among them uploaded in one copy (_upload_many); tensors and
    None pass through untouched (the later _as_dev calls convert / move tensors as before)."""
    host = [i for i, (v, _) in enumerate(pairs) if v is not None and not isinstance(v, torch.Tensor)]
    out = [v for v, _ in pairs]
    if len(host) >= 2:
        up = _upload_many([pairs[i] for i in host], device)
        for i, t in zip(host, up):
            out[i] = t
    return out


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _order(stream) -> None:
    """A caller-supplied stream that is not the current one is ordered behind the current stream: the convenience wrappers
    upload / convert their arguments (and reuse the cached small uploads of _as_dev) on the CURRENT stream."""
    if stream is not None:
        cur = torch.cuda.current_stream()
        if stream != cur:
            stream.wait_stream(cur)


def _stream(stream=None, raw: bool = False):
    """The launch stream as a C handle.  raw=True (InstanceFitter.run: a pure enqueue whose inputs the caller has made ready on
    `stream`, e.g. batches pipelined on several streams) skips the ordering of _order()."""
    if not raw:
        _order(stream)
    s = torch.cuda.current_stream() if stream is None else stream
    return C.c_void_p(s.cuda_stream)


def _record(stream, *tensors):
    """Temporaries allocated on the current stream but consumed by kernels on ``stream``: tell the caching allocator, so the
    blocks are not handed out again while those kernels still read them."""
    if stream is None or stream == torch.cuda.current_stream():
        return
    for t in tensors:   # (tensors; None and anything else is passed over - a caller hands a Depth16 over as its ``data``)
        if isinstance(t, torch.Tensor) and t.is_cuda:
            t.record_stream(stream)


def _int_arg(who: str, name: str, v, lo: int, hi=None) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < lo or (hi is not None and int(v) > hi):
        rng = f">= {lo}" if hi is None else f"in {lo} .. {hi}"
        raise ValueError(f"{who}: {name} must be an int {rng}, not {v!r}")
    return int(v)
