"""The refusal cases of the 13 bit-plane entries of the C ABI (include/la3d.h "masks as bit planes" and later; kernels and checks:
labelany3d_amd/csrc/la3d_bits.hip), shared by tests/test_packer_refusals_contract.py and by whoever records
tests/golden/packer_refusals.json.

Every case starts from a valid call - host pointers into one small aligned buffer, never dereferenced, a NULL stream - and breaks one
argument (or one of the pairs whose precedence is part of the contract).  The valid call itself is never made, and every case is
either refused or has nothing to do: no case reaches a launch, so the cases run on a machine without a GPU.

``run(lib)`` -> [[entry, case, return code, la3d_last_error() or "" for a success], ...] in a fixed order."""
import ctypes as C

F32, F16, BF16 = 0, 1, 2            # LA3D_DTYPE_*
U8, U16, I32, RGB8 = 0, 1, 2, 3     # LA3D_LABEL_*
H, W = 8, 32                         # the valid frame: 8 words a plane
BIG = dict(H=1 << 10, W=1 << 11)     # 2^21 pixels: more than a bit image in LDS holds, fine for the pixel packers


def specs(p):
    """entry -> (argument order, valid values, cases); a case = (name, changed arguments)"""
    uni = dict(B=1, H=H, W=W, W_out=W, bits=p, bits_plane_stride=8)
    frm = dict(frames=p, P=1, H=H, W=W, B=1, bits=p, bits_offsets=p, area=p)

    def sizes(names, wout):
        c = [(f"{n}={v}", {n: v}) for n in names for v in ((-1,) if n in "BP" else (0, -3))]
        return c + ([("W_out<W", dict(W_out=W - 1))] if wout else [])

    def ptrs(required, aligned):
        """required: NULL is refused; aligned: name -> bytes, misaligned by half of them (every weaker rule still holds)"""
        return [(f"{n}=NULL", {n: None}) for n in required] + [(f"{n} misaligned", {n: p + a // 2}) for n, a in aligned.items()]

    nothing = [("B=0", dict(B=0))]
    nothing_p = nothing + [("P=0", dict(P=0)), ("B=0, pointers NULL", dict(B=0, bits=None, frames=None))]
    pix_large = [("frame too large", dict(H=1 << 15, W=1 << 14, W_out=1 << 14)), ("batch too large", dict(B=1 << 25)),
                 ("too large before B=0", dict(H=1 << 15, W=1 << 14, W_out=1 << 14, B=0))]
    pix_stride = [("short source stride", dict(plane_stride=H * W - 1)), ("short bits stride", dict(bits_plane_stride=7)),
                  ("source stride before bits stride", dict(plane_stride=H * W - 1, bits_plane_stride=7))]
    ann = [("W_out no multiple of 32", dict(W_out=40, bits_plane_stride=10)), ("short bits stride", dict(bits_plane_stride=7)),
           ("LDS bound", dict(BIG, W_out=BIG["W"], bits_plane_stride=1 << 16)),
           ("LDS bound before short stride", dict(BIG, W_out=BIG["W"], bits_plane_stride=7)),
           ("LDS bound before B=0", dict(BIG, W_out=BIG["W"], bits_plane_stride=1 << 16, B=0)),
           ("NULL before LDS bound", dict(BIG, W_out=BIG["W"], bits_plane_stride=1 << 16, bits=None)),
           ("misaligned before LDS bound", dict(BIG, W_out=BIG["W"], bits_plane_stride=1 << 16, area=p + 2))]
    ann_f = [("LDS bound", dict(BIG)), ("LDS bound before B=0", dict(BIG, B=0)), ("NULL before LDS bound", dict(BIG, bits=None)),
             ("misaligned before LDS bound", dict(BIG, image_index=p + 2)),
             ("P=0 lets frames be NULL", dict(P=0, frames=None, bits=p + 8)), ("P=0 is no B=0", dict(P=0, bits=None))]
    ann_fp = dict(bits=16, frames=8, bits_offsets=8, image_index=4, area=4)
    lab_dtype = [("dtype=4", dict(dtype=4)), ("dtype=-1", dict(dtype=-1)), ("dtype before sizes", dict(dtype=9, H=0))]
    lg_dtype = [("dtype=3", dict(dtype=3)), ("dtype=-1", dict(dtype=-1)), ("dtype before sizes", dict(dtype=7, H=0))]
    fr_large = [("bounds too large", dict(H=1 << 15, W=1 << 15)), ("too large before B=0", dict(H=1 << 15, W=1 << 15, B=0))]
    mf_args = ["frames", "P", "H", "W", "image_index", "src_offsets", "src_pitch", "B", "bits", "bits_offsets", "area"]
    mf = dict(frm, image_index=p, src_offsets=p, src_pitch=p)
    mf_cases = (sizes("BPHW", False) + fr_large + [("batch too large", dict(H=1 << 14, W=1 << 14, B=1 << 17)),
                                                    ("large bounds, B=0", dict(H=1 << 14, W=1 << 14, B=0))] +
                ptrs(["frames", "image_index", "src_offsets", "bits", "bits_offsets"],
                     dict(bits=4, frames=8, src_offsets=8, bits_offsets=8, image_index=4, src_pitch=4, area=4)) + nothing_p)
    dec = sizes("BHW", False) + [("frame too large", dict(H=1 << 10, W=1 << 11))] + nothing
    return {
        # (the decode pair lives in the same unit: its one-line checks are pinned along)
        "la3d_rle_decode": (["counts", "offsets", "B", "H", "W", "mask_out"], dict(counts=p, offsets=p, B=1, H=H, W=W, mask_out=p),
                            dec + ptrs(["counts", "offsets", "mask_out"], {}) + [("column scan too large for LDS", dict(H=2, W=1 << 19))]),
        "la3d_poly_decode": (["poly_xy", "ring_offsets", "inst_rings", "B", "H", "W", "mask_out"],
                             dict(poly_xy=p, ring_offsets=p, inst_rings=p, B=1, H=H, W=W, mask_out=p),
                             dec + ptrs(["poly_xy", "ring_offsets", "inst_rings", "mask_out"], {})),
        "la3d_pack_mask_bits": (["mask", "plane_stride", "B", "H", "W", "W_out", "bits", "bits_plane_stride"], dict(uni, mask=p, plane_stride=H * W),
                                sizes("BHW", True) + pix_large + ptrs(["mask", "bits"], dict(bits=4)) + pix_stride + nothing +
                                [("any byte address holds a u8 mask", dict(mask=p + 1, B=0))]),
        "la3d_pack_logits_bits": (["logits", "dtype", "plane_stride", "threshold", "B", "H", "W", "W_out", "bits", "bits_plane_stride"],
                                  dict(uni, logits=p, dtype=F16, plane_stride=H * W, threshold=0.0),
                                  lg_dtype + sizes("BHW", True) + pix_large + ptrs(["logits", "bits"], dict(logits=2, bits=4)) + pix_stride + nothing +
                                  [("f32 logits misaligned", dict(dtype=F32, logits=p + 2)), ("bf16 logits misaligned", dict(dtype=BF16, logits=p + 1)),
                                   ("logits misaligned before sizes", dict(logits=p + 1, H=0)), ("logits misaligned, B=0", dict(logits=p + 1, B=0))]),
        "la3d_unpack_mask_bits": (["bits", "bits_plane_stride", "B", "H", "W_in", "W", "mask"], dict(bits=p, bits_plane_stride=8, B=1, H=H, W_in=W, W=W, mask=p),
                                  sizes("BHW", False) + [("W_in<W", dict(W_in=W - 1)), ("frame too large", dict(H=1 << 15, W_in=1 << 14)),
                                                         ("batch too large", dict(B=1 << 25)), ("short bits stride", dict(bits_plane_stride=7))] +
                                  ptrs(["bits", "mask"], dict(bits=4)) + nothing),
        "la3d_mask_stats_bits": (["bits", "bits_plane_stride", "B", "H", "W", "frame_width", "boundary", "stats"],
                                 dict(bits=p, bits_plane_stride=8, B=1, H=H, W=W, frame_width=0, boundary=1, stats=p),
                                 sizes("BHW", False) + [("boundary=-1", dict(boundary=-1)), ("frame_width=-1", dict(frame_width=-1)),
                                                        ("frame_width>W", dict(frame_width=W + 1)), ("short bits stride", dict(bits_plane_stride=7)),
                                                        ("LDS bound", dict(BIG, bits_plane_stride=1 << 16)),
                                                        ("LDS bound before B=0", dict(BIG, bits_plane_stride=1 << 16, B=0))] +
                                 ptrs(["bits", "stats"], dict(bits=4)) + nothing),
        "la3d_pack_rle_bits": (["counts", "offsets", "B", "H", "W", "W_out", "bits", "bits_plane_stride", "area"], dict(uni, counts=p, offsets=p, area=p),
                               sizes("BHW", True) + ann + ptrs(["counts", "offsets", "bits"], dict(bits=4, area=4)) + nothing +
                               [("column scan too large for LDS", dict(H=2, W=1 << 19, W_out=1 << 19, bits_plane_stride=1 << 15))]),
        "la3d_pack_poly_bits": (["poly_xy", "ring_offsets", "inst_rings", "B", "H", "W", "W_out", "bits", "bits_plane_stride", "area"],
                                dict(uni, poly_xy=p, ring_offsets=p, inst_rings=p, area=p),
                                sizes("BHW", True) + ann + ptrs(["poly_xy", "ring_offsets", "inst_rings", "bits"], dict(bits=4, area=4)) + nothing),
        "la3d_pack_rle_bits_frames": (["counts", "offsets", "frames", "P", "H", "W", "image_index", "B", "bits", "bits_offsets", "area"],
                                      dict(frm, counts=p, offsets=p, image_index=p),
                                      sizes("BPHW", False) + ann_f + ptrs(["counts", "offsets", "frames", "image_index", "bits", "bits_offsets"], ann_fp) +
                                      nothing + [("column scan too large for LDS", dict(H=1, W=1 << 20))]),
        "la3d_pack_poly_bits_frames": (["poly_xy", "ring_offsets", "inst_rings", "frames", "P", "H", "W", "image_index", "B", "bits", "bits_offsets", "area"],
                                       dict(frm, poly_xy=p, ring_offsets=p, inst_rings=p, image_index=p),
                                       sizes("BPHW", False) + ann_f +
                                       ptrs(["poly_xy", "ring_offsets", "inst_rings", "frames", "image_index", "bits", "bits_offsets"], ann_fp) + nothing),
        "la3d_pack_label_bits": (["labels", "dtype", "plane_stride", "P", "H", "W", "W_out", "inst_offsets", "inst_label", "B", "bits", "bits_plane_stride", "area"],
                                 dict(uni, labels=p, dtype=U16, plane_stride=H * W, P=1, inst_offsets=p, inst_label=p, area=p),
                                 lab_dtype + sizes("BPHW", True) +
                                 [("frame too large", dict(H=1 << 15, W=1 << 14, W_out=1 << 14)),
                                  ("batch too large", dict(P=1 << 20, H=1 << 12, W=1 << 12, W_out=1 << 12)),
                                  ("too large before B=0", dict(H=1 << 15, W=1 << 14, W_out=1 << 14, B=0))] +
                                 ptrs(["labels", "inst_offsets", "inst_label", "bits"], dict(bits=4, labels=2, inst_offsets=4, inst_label=4, area=4)) +
                                 [("i32 labels misaligned", dict(dtype=I32, labels=p + 2)), ("bits before labels", dict(bits=p + 2, labels=p + 1))] +
                                 pix_stride + nothing + [("P=0", dict(P=0)), ("rgb8 labels at any byte, B=0", dict(dtype=RGB8, labels=p + 1, B=0))]),
        "la3d_pack_label_bits_frames": (["labels", "dtype", "frames", "P", "H", "W", "inst_offsets", "inst_label", "B", "bits", "bits_offsets", "area"],
                                        dict(frm, labels=p, dtype=U16, inst_offsets=p, inst_label=p),
                                        lab_dtype + sizes("BPHW", False) + fr_large +
                                        [("batch too large", dict(P=1 << 17, H=1 << 14, W=1 << 14))] +
                                        ptrs(["labels", "frames", "inst_offsets", "inst_label", "bits", "bits_offsets"],
                                             dict(labels=16, bits=4, frames=8, bits_offsets=8, inst_offsets=4, inst_label=4, area=4)) +
                                        [("labels before bits", dict(labels=p + 8, bits=p + 2))] + nothing_p),
        "la3d_pack_mask_bits_frames": (["mask"] + mf_args, dict(mf, mask=p), mf_cases + ptrs(["mask"], {}) + [("any byte address holds a u8 mask", dict(mask=p + 1, B=0))]),
        "la3d_pack_logits_bits_frames": (["logits", "dtype", "threshold"] + mf_args, dict(mf, logits=p, dtype=F16, threshold=0.0),
                                         lg_dtype + mf_cases + ptrs(["logits"], dict(logits=2)) +
                                         [("f32 logits misaligned", dict(dtype=F32, logits=p + 2)), ("bf16 logits misaligned", dict(dtype=BF16, logits=p + 1)),
                                          ("source before bits", dict(logits=p + 1, bits=p + 2))]),
    }


def run(lib):
    buf = (C.c_double * 64)()
    p = (C.addressof(buf) + 15) & ~15
    out = []
    for entry, (order, valid, cases) in specs(p).items():
        fn = getattr(lib, entry)
        for name, change in cases:
            a = dict(valid, **change)
            assert set(change) <= set(order), (entry, name)
            rc = fn(*[a[k] for k in order], None)
            out.append([entry, name, rc, lib.la3d_last_error().decode() if rc != 0 else ""])
    return out
