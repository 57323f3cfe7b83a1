"""CPU-only contract of the run-length encoder of bit planes (include/la3d.h "bit planes as run lengths": ``la3d_rle_encode_offsets``,
``la3d_rle_encode``, ``la3d_rle_encode_workspace_bytes``, ``la3d_rle_to_string_host``): the exports exist on every layer, the layout of
``la3d_rle_encode_args``, every call-level refusal before any launch (host dummies stand in for the device pointers: a refused call
never touches them), the string helper against the oracle's codec byte for byte, and the Python argument errors before any device
work."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from oracle import la3d_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_C = ("la3d_rle_encode_workspace_bytes", "la3d_rle_encode_offsets", "la3d_rle_encode", "la3d_rle_to_string_host")
NEW_PY = ("RleRuns", "rle_encode_bits", "rle_encode", "rle_encode_bits_frames", "rle_objects", "rle_to_string")


def test_new_symbols_on_every_layer():
    from labelany3d_amd import _lib
    import labelany3d_amd as la
    from labelany3d_amd import masks

    rle_encode = importlib.import_module("labelany3d_amd.rle_encode")   # (the module: ``la.rle_encode`` is the function of that name)
    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    declared = set(re.findall(r"\b(la3d_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_C:
        assert name in declared and hasattr(_lib.lib, name) and name in _lib.EXPORTS, name
    for macro in ("LA3D_RLE_OK 0", "LA3D_RLE_NO_ROOM 1", "LA3D_RLE_MISMATCH 2"):
        assert re.search(r"#define\s+" + macro.replace(" ", r"\s+") + r"\b", hdr), macro
    assert (_lib.RLE_OK, _lib.RLE_NO_ROOM, _lib.RLE_MISMATCH) == (0, 1, 2)
    assert _lib.lib.la3d_version() == 2                      # new exports only: the ABI version stays
    for fn in NEW_PY:
        assert callable(getattr(la, fn)) and fn in la.__all__, fn
    assert la.RleRuns._fields == ("counts", "offsets", "H", "W")   # the 4-tuple pack_rle passes through
    assert masks.rle_encode_bits_frames is rle_encode.rle_encode_bits_frames is la.rle_encode_bits_frames   # (one object: its home, the facade, the package)
    runs = la.RleRuns(np.array([4, 4], np.int32), np.array([0, 2], np.int64), 2, 4)
    assert la.pack_rle(runs) is runs


def test_args_block_layout():
    from labelany3d_amd import _lib

    A = _lib.RleEncodeArgs
    assert C.sizeof(A) == 120
    names = [n for n, _ in A._fields_]
    assert names == ["struct_size", "B", "H", "W", "frame_width", "P", "mask_bits", "bits_plane_stride", "frames", "image_index",
                     "bits_offsets", "runs", "offsets", "counts", "status", "capacity", "workspace", "stream"]
    offs = {n: getattr(A, n).offset for n in names}
    assert offs == dict(struct_size=0, B=4, H=8, W=12, frame_width=16, P=20, mask_bits=24, bits_plane_stride=32, frames=40,
                        image_index=48, bits_offsets=56, runs=64, offsets=72, counts=80, status=88, capacity=96, workspace=104, stream=112)
    # the header declares the fields in this order
    hdr = open(os.path.join(ROOT, "include", "la3d.h")).read()
    body = re.search(r"typedef struct la3d_rle_encode_args \{(.*?)\} la3d_rle_encode_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part).group(1) for stmt in body.split(";") if stmt.strip() for part in stmt.split(",")]
    assert declared == names


def test_workspace_bytes():
    from labelany3d_amd import _lib

    ws = _lib.lib.la3d_rle_encode_workspace_bytes
    for B, H, W in ((0, 480, 640), (-1, 480, 640), (4, 0, 640), (4, -3, 640), (4, 480, 0), (4, 480, -1)):
        assert ws(B, H, W) == 0
    assert ws(1, 480, 640) >= 640 * 8 and ws(1024, 480, 640) >= 1024 * 640 * 8   # two ints per column and instance
    assert ws(3, 1, 1) > 0


def _block(_lib, p, **kw):
    base = dict(struct_size=C.sizeof(_lib.RleEncodeArgs), B=2, H=8, W=64, frame_width=0, P=0, mask_bits=p, bits_plane_stride=0,
                runs=p, offsets=p, counts=p, status=p, capacity=64, workspace=p)
    base.update(kw)
    return _lib.RleEncodeArgs(**base)


def _refused(_lib, fn, a, *words, rc_want=-1):
    f = getattr(_lib.lib, fn)
    rc = f(C.byref(a) if a is not None else None)
    err = _lib.lib.la3d_last_error()
    assert rc == rc_want, (fn, rc, err)
    assert fn.encode() + b":" in err, err
    for w in words:
        assert w in err, err


@pytest.mark.parametrize("fn", ["la3d_rle_encode_offsets", "la3d_rle_encode"])
def test_c_entries_refuse_before_any_launch(fn):
    from labelany3d_amd import _lib

    one = (C.c_double * 64)()
    p = C.addressof(one)   # (16-byte aligned or not, it is 8-byte aligned; p16 below is 16-byte aligned)
    p16 = (p + 15) & ~15
    emit = fn == "la3d_rle_encode"
    bad = lambda *w, rc_want=-1, **kw: _refused(_lib, fn, _block(_lib, p16, **kw), *w, rc_want=rc_want)   # noqa: E731
    _refused(_lib, fn, None, b"struct_size")
    bad(b"struct_size", struct_size=8)
    bad(b"struct_size", struct_size=0)
    for k in ("B", "H", "W", "P"):
        bad(b"negative sizes", **{k: -1})
    bad(b"frame_width", frame_width=-1)
    bad(b"frame_width", frame_width=65)
    bad(b"bits_plane_stride", bits_plane_stride=-1)
    bad(b"bits_plane_stride", bits_plane_stride=15)                       # below the 16 words of an 8 x 64 plane
    bad(b"H, W > 0", H=0)
    bad(b"H, W > 0", W=0)
    bad(b"bits_offsets without frames", bits_offsets=p16)
    bad(b"frames without image_index", frames=p16, bits_offsets=p16)
    bad(b"must be 0 in a frames call", frames=p16, bits_offsets=p16, image_index=p16, frame_width=32)
    bad(b"must be 0 in a frames call", frames=p16, bits_offsets=p16, image_index=p16, bits_plane_stride=16)
    bad(b"offsets", offsets=None)
    bad(b"offsets", offsets=p16 + 4)
    bad(b"NULL", mask_bits=None)
    bad(b"NULL", workspace=None)
    bad(b"NULL", frames=p16, image_index=p16, bits_offsets=None)
    bad(b"4-byte", mask_bits=p16 + 2)
    bad(b"8-byte", workspace=p16 + 4)
    bad(b"16-byte", frames=p16, image_index=p16, bits_offsets=p16, mask_bits=p16 + 4)
    bad(b"8-byte", frames=p16 + 4, image_index=p16, bits_offsets=p16)
    bad(b"8-byte", frames=p16, image_index=p16, bits_offsets=p16 + 4)
    bad(b"4-byte", frames=p16, image_index=p16 + 2, bits_offsets=p16)
    if emit:
        bad(b"capacity", capacity=-1)
        bad(b"NULL", counts=None)
        bad(b"NULL", status=None)
        bad(b"4-byte", counts=p16 + 1)
        bad(b"4-byte", status=p16 + 2)
    else:
        bad(b"NULL", runs=None)
        bad(b"4-byte", runs=p16 + 2)
    # the bit image lives in LDS: H * W (frames: H * roundup32(W)) <= 1048576
    bad(b"1048576", H=1024, W=1056, rc_want=-2)
    bad(b"1048576", H=1, W=1048577, rc_want=-2)
    bad(b"1048576", H=1024, W=1025, frames=p16, image_index=p16, bits_offsets=p16, rc_want=-2)
    # no instances: both stages succeed without a device as far as nothing is launched (the first stage writes offsets[0] on a stream)
    if emit:
        assert _lib.lib.la3d_rle_encode(C.byref(_block(_lib, p16, B=0, mask_bits=None, workspace=None, counts=None, status=None))) == 0


def _c_to_string(_lib, counts, cap=None):
    c = np.ascontiguousarray(counts, dtype=np.int32)
    cap = 7 * len(c) + 1 if cap is None else cap
    buf = C.create_string_buffer(max(cap, 1))
    n = _lib.lib.la3d_rle_to_string_host(c.ctypes.data if len(c) else None, len(c), buf, cap)
    return n, buf.raw[:max(n, 0)]


def _count_lists():
    """200 seeded count lists: zero counts, counts >= 2^15, negative differences to the count two places back, lengths 0 to 3 (the
    prefix stored without a difference)."""
    rs = np.random.RandomState(20)
    lists = [[], [0], [7], [0, 0], [5, 0], [0, 307200], [1, 2, 3], [0, 0, 0], [40000, 1, 2], [1 << 20, 0, 1 << 20, 0, 1]]
    while len(lists) < 200:
        n = int(rs.randint(0, 40))
        kind = rs.randint(0, 4)
        if kind == 0:
            c = rs.randint(0, 50, n)
        elif kind == 1:
            c = rs.randint(0, 1 << 20, n)
        elif kind == 2:
            c = np.where(rs.rand(n) < 0.3, 0, rs.randint(1 << 15, 1 << 19, n))
        else:   # big then small two places on: negative differences
            c = np.where(np.arange(n) % 4 < 2, rs.randint(1 << 15, 1 << 20, n), rs.randint(0, 31, n))
        lists.append([int(x) for x in c])
    assert any(len(c) > 3 and any(c[i] - c[i - 2] < 0 for i in range(3, len(c))) for c in lists)
    assert any(0 in c for c in lists) and any(max(c, default=0) >= 1 << 15 for c in lists)
    assert {0, 1, 2, 3} <= {len(c) for c in lists}
    return lists


def test_to_string_host_equals_oracle_byte_for_byte(golden):
    from labelany3d_amd import _lib, rle_from_string, rle_to_string

    g = golden("g8_masks.npz")
    offs = np.concatenate([[0], np.cumsum(g["lens"])])
    lists = [g["counts"][offs[i]:offs[i + 1]].tolist() for i in range(len(g["lens"]))] + _count_lists()
    for c in lists:
        want = O.rle_to_string(c)
        n, got = _c_to_string(_lib, c)
        assert n == len(want) and got == want, (c, got, want)
        assert rle_to_string(c) == want.decode("ascii")
        np.testing.assert_array_equal(rle_from_string(got), np.asarray(c, np.int32))   # from_string(to_string(c)) == c
        # a cap that fits exactly succeeds, one byte less is refused
        assert _c_to_string(_lib, c, cap=len(want)) == (len(want), want)
        if len(want):
            assert _c_to_string(_lib, c, cap=len(want) - 1)[0] == -1
    assert _lib.lib.la3d_rle_to_string_host(None, 3, C.create_string_buffer(8), 8) == -1
    assert _lib.lib.la3d_rle_to_string_host(None, -1, C.create_string_buffer(8), 8) == -1


def test_python_entries_check_arguments_before_any_device_work(monkeypatch):
    import torch

    import labelany3d_amd as la

    def no_device(*a, **k):
        raise AssertionError("the entry touched the device before it checked its arguments")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    words = torch.zeros((2, 16), dtype=torch.int32)
    for notbits in (words, (words, 8, 64, 64), None, [1, 2, 3], np.zeros((2, 8, 64), bool)):
        with pytest.raises(ValueError, match="MaskBits"):
            la.rle_encode_bits(notbits)
    mb = la.MaskBits(words, 8, 64, 64)
    for cap in (-1, 2.5, "7", True):
        with pytest.raises(ValueError, match="capacity"):
            la.rle_encode_bits(mb, capacity=cap)
        with pytest.raises(ValueError, match="capacity"):
            la.rle_encode_bits_frames(None, None, capacity=cap)
    with pytest.raises(ValueError, match="GPU"):
        la.rle_encode_bits(mb, capacity=8)                      # host planes: refused by the layout check, no device asked
    with pytest.raises(ValueError, match="frame_width"):
        la.rle_encode_bits(la.MaskBits(words, 8, 64, 65), capacity=8)
    with pytest.raises(ValueError, match="frames must be"):
        la.rle_encode_bits_frames(object(), None)
    pf = la.pack_frames([np.ones((8, 20), np.float32), np.ones((5, 40), np.float32)], device="cpu")
    with pytest.raises(ValueError, match="FrameBits"):
        la.rle_encode_bits_frames(pf, mb)
    with pytest.raises(ValueError):
        la.rle_objects((words, words))                          # (counts, offsets) without sizes
    # rle_objects on host arrays: the JSON objects, plain and compressed
    runs = la.RleRuns(np.array([3, 2, 3, 0, 8], np.int32), np.array([0, 3, 5], np.int64), 2, 4)
    assert la.rle_objects(runs) == [{"size": [2, 4], "counts": [3, 2, 3]}, {"size": [2, 4], "counts": [0, 8]}]
    assert la.rle_objects(runs, compress=True) == [{"size": [2, 4], "counts": O.rle_to_string([3, 2, 3]).decode()},
                                                   {"size": [2, 4], "counts": O.rle_to_string([0, 8]).decode()}]
