"""The rows a frames call refuses on the device, one fault per row: the case table the refused-row tests of every frames-form entry
outside the fit share (opening, components, run-length encoder, point clouds, overlap), so that a change of the la3d_frame contract
or of the plane locator (la3d_bitplanes.hpp: frames_prologue, frames_source, frames_dest) meets the same faults everywhere.

The discipline of every user: the frame table has a VALID pad row in front (index -1) and behind (index P), the buffers have ``PAD``
words in front and behind, and every bad offset stays inside the test's own allocation - a defect then uses a valid frame or reads
and writes the test's own words, and shows as a changed word or a wrong sentinel, never as a fault.  No case relies on a fault."""
from types import SimpleNamespace

import numpy as np

GOOD = [(33, 47), (40, 32), (8, 33)]             # the images good rows belong to: (H, W) unpadded
H, W = 40, 64                                    # the bounds of the good frames
PAD_FRAME = (0, 8, 32, 32, 0)                    # rows -1 and P of the table: a valid frame, which nothing may use
SLOT, PAD = 128, 64                              # words: a slot holds the plane of every row, bad ones included; pad around a buffer
# la3d_frame rows that break the contract, one rule each: (depth_offset, H, W = pitch, frame_width, reserved)
FRAME_FAULTS = [
    ("pitch 48: not a multiple of 32", (0, 8, 48, 40, 0)),
    ("H above the bound", (0, 41, 64, 40, 0)),
    ("W above the bound", (0, 8, 96, 40, 0)),
    ("frame_width 0", (0, 8, 32, 0, 0)),
    ("frame_width > W", (0, 8, 32, 33, 0)),
    ("depth_offset negative", (-4, 8, 32, 32, 0)),
    ("depth_offset not a multiple of 4", (2, 8, 32, 32, 0)),
]
INDEX_FAULTS = ["image index -1", "image index P"]
OFFSET_FAULTS = ["plane offset negative", "plane offset not a multiple of 4"]
END_FAULT = "plane ends one word past the buffer"
P = len(GOOD) + len(FRAME_FAULTS)                # images of the table


def padded(w):
    return (w + 31) // 32 * 32


def plane_words(h, w):
    return h * padded(w) // 32


def frame_table(depth_offsets=(0, 0, 0)):
    """the table with its two pad rows: row 1 + p is image p; the good images first, then one image per FRAME_FAULTS row"""
    from labelany3d_amd.frames import FRAME_DTYPE

    t = np.zeros(P + 2, FRAME_DTYPE)
    t[0] = t[P + 1] = PAD_FRAME
    for p, (h, w) in enumerate(GOOD):
        t[1 + p] = (depth_offsets[p], h, padded(w), w, 0)
    for j, (_, row) in enumerate(FRAME_FAULTS):
        t[1 + len(GOOD) + j] = row
    return t


def case(end_check, extra=(), depth_offsets=(0, 0, 0)):
    """rows = [(image, fault or None)], a good row first and last; ``end_check``: the entry takes the length of its buffer; ``extra``:
    further (image, fault) rows of the caller's own (faults of an output, say), put in front of the last good row.  Plane n lies
    ``offsets[n]`` words into a buffer of ``words`` words: row n has slot n, but for the offset faults."""
    bad_image = {name: len(GOOD) + j for j, (name, _) in enumerate(FRAME_FAULTS)}
    f = [name for name, _ in FRAME_FAULTS]
    rows = [(0, None), (-1, INDEX_FAULTS[0]), (1, None), (P, INDEX_FAULTS[1]), (bad_image[f[0]], f[0]), (2, None)]
    rows += [(bad_image[x], x) for x in f[1:5]] + [(0, None)] + [(bad_image[x], x) for x in f[5:]]
    rows += [(1, OFFSET_FAULTS[0]), (1, None), (2, OFFSET_FAULTS[1])]
    if end_check:
        rows.append((0, END_FAULT))
    rows += list(extra) + [(2, None)]
    B = len(rows)
    words = B * SLOT + 1
    offsets = np.arange(B, dtype=np.int64) * SLOT
    for n, (img, bad) in enumerate(rows):
        if bad == OFFSET_FAULTS[0]:
            offsets[n] = -4
        elif bad == OFFSET_FAULTS[1]:
            offsets[n] += 2
        elif bad == END_FAULT:
            offsets[n] = words - plane_words(*GOOD[img]) + 1
            assert offsets[n] % 4 == 0 and offsets[n] >= 0
    assert rows[0][1] is None and rows[-1][1] is None and B <= 24 and -4 >= -PAD
    return SimpleNamespace(rows=rows, B=B, P=P, H=H, W=W, words=words, offsets=offsets, table=frame_table(depth_offsets),
                           good=[n for n, (_, bad) in enumerate(rows) if bad is None],
                           refused=[n for n, (_, bad) in enumerate(rows) if bad is not None],
                           image_index=np.array([img for img, _ in rows], np.int32))


def input_words(c, rs, plane_of):
    """the input buffer with its pads: garbage wherever no plane lies, the words ``plane_of(n, h, w)`` gives for every good row n"""
    buf = rs.randint(0, 2 ** 32, PAD + c.words + PAD, dtype=np.uint64).astype(np.uint32)
    for n in c.good:
        wds = plane_of(n, *GOOD[c.rows[n][0]])
        assert len(wds) == plane_words(*GOOD[c.rows[n][0]]) <= SLOT
        buf[PAD + c.offsets[n]:PAD + c.offsets[n] + len(wds)] = wds
    return buf


def on_device(c, inbuf):
    """-> the device tensors of a call: ``table`` (P, 6) and ``bits`` (c.words,) are VIEWS into allocations that carry the pads (the
    allocations are kept beside them), ``offsets``, ``image_index``"""
    import torch

    from labelany3d_amd.frames import table_words

    table_all = torch.as_tensor(table_words(c.table), device="cuda")
    bits_all = torch.as_tensor(inbuf.view(np.int32), device="cuda")
    d = SimpleNamespace(table_all=table_all, table=table_all[1:1 + c.P], bits_all=bits_all, bits=bits_all[PAD:PAD + c.words],
                        offsets=torch.as_tensor(c.offsets, device="cuda"), image_index=torch.as_tensor(c.image_index, device="cuda"))
    assert d.table.data_ptr() == table_all.data_ptr() + 24 and d.bits.data_ptr() % 16 == 0 and d.table.is_contiguous()
    return d


def frame_bits(la, c, d, rows=None):
    """the FrameBits of the call (``rows``: of these rows only - the call without the bad rows)"""
    import torch

    sel = slice(None) if rows is None else torch.as_tensor(np.asarray(rows, np.int64), device="cuda")
    n = c.B if rows is None else len(rows)
    return la.FrameBits(d.bits, d.offsets[sel].contiguous(), d.image_index[sel].contiguous(), torch.zeros(n, dtype=torch.int32, device="cuda"),
                        c.table[1:1 + c.P], c.H, c.W)


def frame_grid(la, c, d):
    """the ``frames`` of an entry that reads only the frame table"""
    return la.FrameGrid(d.table, c.table[1:1 + c.P], c.H, c.W, [(int(r["H"]), int(r["frame_width"])) for r in c.table[1:1 + c.P]])
