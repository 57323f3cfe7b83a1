"""The staging paths of the frames packers that exist on a device only (labelany3d_amd/frames.py ``_stage_ragged``): device sources
(zeros on the device, one device copy per piece) and host sources through a pinned staging tensor (one asynchronous upload) give, for
``pack_frames``, ``pack_label_frames`` and ``pack_mask_frames``, the bytes of the ``device="cpu"`` layout that
tests/test_frames_staging_contract.py holds to its NumPy restatement.  That device stacks which can be read in place are NOT staged -
``data`` aliases the lowest source, ``sources`` keeps them - is asserted by
tests/test_gpu_frames_masks.py::test_device_stacks_are_read_in_place."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(8, 32), (5, 33), (16, 64)]
KINDS = ["frames-f32", "frames-u16", "labels-u16", "labels-rgb", "masks-bool", "masks-f16"]


@pytest.fixture(scope="module")
def la():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import labelany3d_amd

    return labelany3d_amd


def _inputs(la, kind):
    """-> (pack(inputs, **kw) -> the packed result, its flat tensor's field, host inputs, the stored torch dtype)"""
    import torch

    rs = np.random.RandomState(KINDS.index(kind))
    if kind == "frames-f32":
        return la.pack_frames, "depth", [rs.rand(h, w).astype(np.float32) for h, w in SIZES], torch.float32
    if kind == "frames-u16":
        maps = [rs.randint(0, 65536, (h, w)).astype(np.uint16) for h, w in SIZES]
        return (lambda x, **kw: la.pack_frames(x, dtype="u16", **kw)), "data", maps, torch.uint16
    if kind == "labels-u16":
        return la.pack_label_frames, "data", [rs.randint(0, 65536, (h, w)).astype(np.uint16) for h, w in SIZES], torch.int16
    if kind == "labels-rgb":
        maps = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
        return (lambda x, **kw: la.pack_label_frames(x, rgb=True, **kw)), "data", maps, torch.uint8
    if kind == "masks-bool":
        return la.pack_mask_frames, "data", [rs.rand(n, h, w) > 0.5 for n, (h, w) in zip((2, 0, 3), SIZES)], torch.uint8
    return la.pack_mask_frames, "data", [rs.randn(n, h, w).astype(np.float16) for n, (h, w) in zip((2, 0, 3), SIZES)], torch.float16


def _bytes(t):
    import torch

    return t.cpu().view(torch.uint8).numpy().tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_device_and_pinned_staging_give_the_host_layout(la, kind):
    import torch

    pack, field, host, tdt = _inputs(la, kind)
    want = pack(host, device="cpu")
    flat = getattr(want, field)
    n = flat.numel()
    # device sources; the last one strided (a transposed view), so that a mask stack cannot be read in place and is staged too
    dev = [torch.as_tensor(m, device="cuda") for m in host]
    dev[-1] = dev[-1].transpose(-1, -2).contiguous().transpose(-1, -2) if kind.startswith("masks") else dev[-1]
    got = pack(dev)
    assert getattr(got, field).is_cuda and getattr(got, field).dtype == tdt and not getattr(got, "sources", ())
    assert _bytes(getattr(got, field)) == _bytes(flat)
    # device and host sources in one call
    got = pack([dev[0]] + host[1:])
    assert getattr(got, field).is_cuda and _bytes(getattr(got, field)) == _bytes(flat)
    # host sources through a pinned staging tensor that holds stale bytes
    pinned = torch.empty(n + 8, dtype=tdt).pin_memory()
    pinned.view(torch.uint8).fill_(0x5a)
    got = pack(host, pinned=pinned)
    torch.cuda.synchronize()
    assert getattr(got, field).is_cuda and getattr(got, field).numel() == n and _bytes(getattr(got, field)) == _bytes(flat)
    assert _bytes(pinned[:n]) == _bytes(flat) and (pinned[n:].view(torch.uint8) == 0x5a).all()      # it WAS the staging buffer
    for a, b in zip(got, want):                                               # the table, the offsets, the bounds: as on the host
        if isinstance(a, torch.Tensor):
            assert a.is_cuda and _bytes(a) == _bytes(b)
        elif isinstance(a, np.ndarray):
            assert a.tobytes() == b.tobytes()
        else:
            assert a == b
