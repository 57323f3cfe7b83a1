"""CPU-only contract of the staging the three frames packers share (labelany3d_amd/frames.py: ``_stage_ragged``, ``table_words``):
``pack_frames``, ``pack_label_frames`` and ``pack_mask_frames`` state ONE table for equal sizes, every buffer is the NumPy
restatement below - each map at its table offset, zero padding, zero tail, the packer's own minimum length -, a staging tensor is
used exactly when its dtype and size fit, and arrays and tensors give the same bytes."""
import numpy as np
import pytest

SIZES = [(1, 1), (5, 33), (8, 32), (3, 64)]          # one pixel; a pitch of 64 for 33 columns; no padding at all; a second row of tiles
STACK_COUNTS = [2, 0, 1, 3]                          # planes per image of the mask stacks: image 1 has none
KINDS = ["frames-f32", "frames-f16", "frames-u16", "labels-u8", "labels-u16", "labels-i32", "labels-rgb", "masks-bool", "masks-f16"]


def _pitch(w):
    return (w + 31) // 32 * 32


def _ragged(maps, sizes, c, floor):
    """maps of (h, w * c) stored elements under the frame table of ``sizes``: planes back to back at pitch ``_pitch(w)``"""
    total = sum(h * _pitch(w) for h, w in sizes)
    out = np.zeros(max(total, floor) * c, maps[0].dtype if maps else np.uint8)
    off = 0
    for m, (h, w) in zip(maps, sizes):
        out[off * c:(off + h * _pitch(w)) * c].reshape(h, _pitch(w) * c)[:, :w * c] = m.reshape(h, w * c)
        off += h * _pitch(w)
    return out


def _case(kind, sizes):
    """-> (pack(inputs, pinned) -> flat tensor, the inputs as NumPy arrays, the bytes the buffer must hold, the stored torch dtype -
    uint8 where no label map / mask stack says another)"""
    import torch

    from labelany3d_amd import pack_frames, pack_label_frames, pack_mask_frames

    rs = np.random.RandomState(len(sizes) * 16 + KINDS.index(kind))
    what, elem = kind.split("-")
    if what == "frames":
        ndt, tdt, dtype = {"f32": (np.float32, torch.float32, None), "f16": (np.float16, torch.float16, "f16"),
                           "u16": (np.uint16, torch.uint16, "u16")}[elem]
        maps = [(rs.rand(h, w) * 60000 + 1).astype(ndt) for h, w in sizes]
        want = _ragged(maps, sizes, 1, 4) if maps else np.zeros(4, ndt)
        return (lambda x, pinned=None: getattr(pack_frames(x, device="cpu", pinned=pinned, dtype=dtype), "depth" if dtype is None else "data"),
                maps, want, tdt)
    if what == "labels":
        ndt, tdt, c = {"u8": (np.uint8, torch.uint8, 1), "u16": (np.uint16, torch.int16, 1), "i32": (np.int32, torch.int32, 1),
                       "rgb": (np.uint8, torch.uint8, 3)}[elem]
        maps = [rs.randint(0, 250, (h, w) + ((3,) if c == 3 else ())).astype(ndt) * (ndt(257) if elem == "u16" else ndt(1)) for h, w in sizes]
        want = _ragged(maps, sizes, c, 16) if maps else np.zeros(16 * c, np.uint8)
        return lambda x, pinned=None: pack_label_frames(x, rgb=c == 3, device="cpu", pinned=pinned).data, maps, want, tdt if maps else torch.uint8
    ndt, tdt = {"bool": (np.bool_, torch.uint8), "f16": (np.float16, torch.float16)}[elem]
    stacks = [(rs.rand(n, h, w) > 0.5) if ndt is np.bool_ else rs.randn(n, h, w).astype(ndt) for n, (h, w) in zip(STACK_COUNTS, sizes)]
    planes = np.concatenate([s.reshape(-1) for s in stacks]) if stacks else np.zeros(0, np.uint8)   # dense: no pitch, no padding
    want = np.zeros(max(planes.size, 16), np.uint8 if ndt is np.bool_ or not stacks else ndt)
    want[:planes.size] = planes
    return lambda x, pinned=None: pack_mask_frames(x, device="cpu", pinned=pinned).data, stacks, want, tdt if stacks else torch.uint8


def _bytes(t):
    import torch

    return t.view(torch.uint8).numpy()


@pytest.mark.parametrize("sizes", [SIZES, []], ids=["four-sizes", "empty"])
def test_the_three_packers_state_one_table(sizes):
    from labelany3d_amd import pack_frames, pack_label_frames, pack_mask_frames

    pf = pack_frames([np.ones(s, np.float32) for s in sizes], device="cpu")
    pl = pack_label_frames([np.ones(s, np.uint8) for s in sizes], device="cpu")
    pm = pack_mask_frames([np.ones((n,) + s, bool) for n, s in zip(STACK_COUNTS, sizes)], device="cpu")
    want = np.zeros((len(sizes), 6), np.int32)                       # la3d_frame: int64 offset, H, pitch, W, reserved
    off = 0
    for p, (h, w) in enumerate(sizes):
        want[p] = (off & 0xffffffff, off >> 32, h, _pitch(w), w, 0)
        off += h * _pitch(w)
    for got in (pf, pl, pm):
        assert got.table_host.tobytes() == pf.table_host.tobytes() and got.table_host.dtype == pf.table_host.dtype
        assert tuple(got.table.shape) == (len(sizes), 6) and got.table.numpy().tobytes() == want.tobytes()
        assert got.table_host.tobytes() == want.tobytes()
        assert (got.H, got.W) == (max((h for h, _ in sizes), default=0), max((_pitch(w) for _, w in sizes), default=0))
        assert got.sizes == list(sizes)


@pytest.mark.parametrize("sizes", [SIZES, []], ids=["four-sizes", "empty"])
@pytest.mark.parametrize("kind", KINDS)
def test_buffer_is_the_numpy_restatement(kind, sizes):
    import torch

    pack, maps, want, tdt = _case(kind, sizes)
    flat = pack(maps)
    assert flat.dtype == tdt and flat.dim() == 1 and flat.numel() == want.size
    assert _bytes(flat).tobytes() == want.tobytes()
    # host tensors, and a mix of arrays and tensors, give the bytes of the arrays
    tensors = [torch.as_tensor(m) for m in maps]
    assert _bytes(pack(tensors)).tobytes() == want.tobytes()
    assert _bytes(pack([t if i % 2 else m for i, (m, t) in enumerate(zip(maps, tensors))])).tobytes() == want.tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_staging_tensor_is_used_when_dtype_and_size_fit(kind):
    import torch

    pack, maps, want, tdt = _case(kind, SIZES)
    n = want.size

    def stage(numel, dtype):
        t = torch.empty(numel, dtype=dtype)
        t.view(torch.uint8).fill_(0x5a)                               # stale bytes: padding and tail must be zeroed by the packer
        return t

    fits = stage(n + 100, tdt)
    flat = pack(maps, fits)
    assert flat.data_ptr() == fits.data_ptr() and flat.numel() == n and _bytes(flat).tobytes() == want.tobytes()
    assert (_bytes(fits[n:]) == 0x5a).all()                           # nothing past the packed size is written
    exact = stage(n, tdt)
    assert pack(maps, exact).data_ptr() == exact.data_ptr() and _bytes(exact).tobytes() == want.tobytes()
    other = torch.float64 if tdt != torch.float64 else torch.float32
    for unfit in (stage(n - 1, tdt), stage(n + 100, other)):          # too small; another dtype: ignored, same contents
        flat = pack(maps, unfit)
        assert flat.data_ptr() != unfit.data_ptr() and flat.dtype == tdt and _bytes(flat).tobytes() == want.tobytes()
        assert (_bytes(unfit) == 0x5a).all()
