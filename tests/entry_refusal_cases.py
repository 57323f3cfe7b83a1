"""The refusal cases of the C entries outside the bit-plane units (include/la3d.h; checks: labelany3d_amd/csrc/la3d.hip - every fit
entry and fit_dispatch behind them -, la3d_instance.hip - what the instance engine refuses before its launch -, la3d_points.hip,
la3d_masks.hip, la3d_consumers.hip, la3d_depth16.hip, la3d_align.hip), shared by tests/test_entry_refusals_contract.py and by whoever
records tests/golden/entry_refusals.json.  tests/packer_refusal_cases.py holds the cases of the bit-plane entries.

Every case starts from a valid call - pointers into one small aligned buffer, never dereferenced, a NULL stream - and breaks one
argument (or one of the pairs whose precedence is part of the contract).  The valid call itself is never made, and every case is
either refused or has nothing to do: no case reaches a launch, an allocation or hipGetDevice, so the cases run on a machine without
a GPU.  la3d_fit_annotations_host alone READS host arrays before it touches the device (image_index, the offsets): those cases
point at real arrays.

An entry that takes an argument block (la3d_fit_args, la3d_align_ransac_args) has "args" in its argument order: the cases change
fields of a valid block, and "args" = None passes no block at all.  "depth16" stands for a la3d_depth16 block, built from the d_*
values (None: no block).

``run(lib)`` -> [[entry, case, return code, la3d_last_error() or "" for a success], ...] in a fixed order."""
import ctypes as C

F32, F16, BF16, U16 = 0, 1, 2, 3     # LA3D_DTYPE_*
PCA, HULL = 0, 1                     # LA3D_METHOD_*
INSTANCE = 1                         # LA3D_ENGINE_INSTANCE
H, W = 8, 32                         # the valid frame: 8 words a plane
V1 = 200                             # la3d_fit_args as first published: every field up to `stream`
BIG = dict(H=1024, W=2048)           # 2^21 pixels: more than a bit image in LDS holds
NOLDS = dict(H=1025, W=1024)         # a u8 frame whose bit image stays out of LDS (the call is fine without it)
WIDE = dict(H=8, W=8192)             # a frames bound of 256 tiles a row: outside the tiled form, the bit image fits
FILTER = dict(filter_boundary=10, filter_min_area=100, filter_max_edge=10)
NAN, INF = float("nan"), float("inf")


def _blocks():
    from labelany3d_amd._lib import AlignRansacArgs, FitArgs

    fit = ("la3d_fit_instances_ex", "la3d_fit_instances_bits", "la3d_fit_instances_depth16", "la3d_fit_instances_frames",
           "la3d_fit_instances_frames_depth16", "la3d_fit_instances_frames_bits", "la3d_fit_annotations_host")
    return dict({e: FitArgs for e in fit}, la3d_align_ransac_batch=AlignRansacArgs)


def specs(p, host):
    """entry -> (argument order, valid values, cases); a case = (name, changed arguments).  p: the fake pointer; host: real arrays
    (name -> address) for the one entry that reads some."""
    from labelany3d_amd._lib import AlignRansacArgs, FitArgs

    FULL = C.sizeof(FitArgs)

    def null(*names):
        return [(f"{n}=NULL", {n: None}) for n in names]

    # ---- what fit_dispatch refuses, for every fit entry: the compound rule, the method, B = 0, the workspace ----
    def dispatch(block):
        c = null("K", "out", "status") + [(f"{n}={v}", {n: v}) for n, v in (("B", -1), ("H", 0), ("H", -3), ("W", 0), ("W", -32), ("k_stride", 8), ("k_stride", -9))]
        c += [("H*W > 2^28", dict(H=16385, W=16384)), ("H*W > 2^28 before B=0", dict(H=16385, W=16384, B=0)),
              ("B=0", dict(B=0)), ("B=0 before workspace", dict(B=0, workspace=None)),
              ("workspace=NULL", dict(workspace=None)), ("workspace misaligned", dict(workspace=p + 4)),
              ("bad argument before workspace", dict(K=None, workspace=None))]
        if block:
            c += [("method=2", dict(method=2)), ("method=-1", dict(method=-1)), ("bad argument before method", dict(B=-1, method=2)),
                  ("method before B=0", dict(method=2, B=0)), ("method before workspace", dict(method=2, workspace=None))]
        return c

    hull_ws = [("hull workspace=NULL", dict(method=HULL, workspace=None)), ("hull workspace misaligned", dict(method=HULL, workspace=p + 4))]
    options = ([("proj without image size", dict(proj=p)), ("proj with image_width only", dict(proj=p, image_width=640.0))] +
               [(f"{n}={v}", {n: v}) for n, v in (("opt_engine", -1), ("opt_engine", 6), ("opt_launch_order", -1), ("opt_launch_order", 3),
                                                  ("opt_build", -1), ("opt_build", 3))] +
               [("proj before opt", dict(proj=p, opt_engine=-1)), ("options before bad argument", dict(opt_engine=-1, B=-1)),
                ("options before B=0", dict(opt_build=3, B=0))])
    # (the frames entries set the image size themselves: only the opt_* rule is left)
    options_f = [c for c in options if not c[0].startswith("proj")] + [("proj needs no image size", dict(proj=p, workspace=None))]
    size = [("args=NULL", dict(args=None)), ("struct_size=0", dict(struct_size=0)), (f"struct_size={V1 - 1}", dict(struct_size=V1 - 1)),
            ("a block as first published, B=0", dict(struct_size=V1, B=0, method=7)),
            ("a block as first published: method is not read", dict(struct_size=V1, method=7, workspace=None)),
            ("a longer block is read", dict(struct_size=FULL + 8, B=-1))]

    # ---- the legacy entries: positional arguments ----
    head = ["depth", "depth_plane_stride", "image_index"]
    cam = ["K", "k_stride", "ground", "sample_idx", "B", "H", "W"]
    tail = ["out", "status", "aux", "workspace", "stream"]
    filt = ["boundary", "min_area", "max_edge", "out", "status", "aux", "stats", "workspace", "stream"]
    leg = dict(depth=p, depth_plane_stride=0, image_index=None, K=p, k_stride=0, ground=None, sample_idx=None, B=1, H=H, W=W,
               out=p, status=p, aux=None, workspace=p, stream=None, boundary=10, min_area=100, max_edge=10, stats=None)
    leg_common = null("depth") + [("depth_plane_stride=-1", dict(depth_plane_stride=-1))] + dispatch(False)
    leg_lds = [("LDS bound", dict(BIG)), ("workspace before LDS bound", dict(BIG, workspace=None)), ("B=0 before LDS bound", dict(BIG, B=0))]
    leg_filter = [("boundary=-1", dict(boundary=-1)), ("boundary=-1, B=0", dict(boundary=-1, B=0)),
                  ("workspace before filter", dict(boundary=-1, workspace=None)), ("filter before LDS bound", dict(BIG, boundary=-1))]
    rle_m, poly_m = dict(rle_counts=p, rle_offsets=p), dict(poly_xy=p, ring_offsets=p, inst_rings=p)
    rle_c = [("rle_counts=NULL", dict(rle_counts=None)), ("rle_counts=NULL, B=0", dict(rle_counts=None, B=0)), ("rle_offsets=NULL", dict(rle_offsets=None)),
             ("rle_offsets=NULL, B=0", dict(rle_offsets=None, B=0))]
    poly_c = (null("poly_xy", "ring_offsets", "inst_rings") +
              [("poly_xy=NULL, B=0", dict(poly_xy=None, B=0)), ("inst_rings=NULL, B=0", dict(inst_rings=None, B=0)),
               ("no polygon pointer, B=0", dict(poly_xy=None, ring_offsets=None, inst_rings=None, B=0))])

    # ---- la3d_fit_instances_ex: a block; the valid call gives run lengths ----
    blk = dict(struct_size=FULL, B=1, H=H, W=W, depth=p, K=p, out=p, status=p, workspace=p)
    ex_v = dict(blk, **rle_m)
    u8 = dict(rle_counts=None, rle_offsets=None, mask=p)
    poly = dict(rle_counts=None, rle_offsets=None, **poly_m)
    sample_nolds = dict(u8, **NOLDS, sample_idx=p)     # reference-subsample mode on a frame whose bit image stays out of LDS
    ex_cases = (size + [("struct_size before kinds", dict(struct_size=0, mask=p))] +
                [("two kinds", dict(mask=p)), ("three kinds", dict(mask=p, **poly_m)), ("no kind", dict(rle_counts=None)),
                 ("no kind, B=0", dict(rle_counts=None, B=0)), ("two kinds, B=0", dict(mask=p, B=0)),
                 ("kinds before polygon rule", dict(poly_xy=p)),
                 ("polygons without ring_offsets", dict(poly, ring_offsets=None)), ("polygons without inst_rings", dict(poly, inst_rings=None)),
                 ("polygon rule holds for B=0", dict(poly, inst_rings=None, B=0)), ("polygon rule before proj", dict(poly, ring_offsets=None, proj=p))] +
                options + null("depth") + [("depth_plane_stride=-1", dict(depth_plane_stride=-1)), ("rle_offsets=NULL", dict(rle_offsets=None))] +
                dispatch(True) + hull_ws +
                [("frame_width=-1", dict(frame_width=-1)), ("frame_width>W", dict(frame_width=W + 1)), ("frame_width, W no multiple of 32", dict(frame_width=20, W=48)),
                 ("frame_width with u8 planes", dict(u8, frame_width=20)), ("frame_width=W is no padding", dict(u8, **FILTER, frame_width=W)),
                 ("workspace before frame_width", dict(frame_width=-1, workspace=None)), ("frame_width before filter", dict(u8, **FILTER, frame_width=20)),
                 ("frame_width before LDS bound", dict(BIG, frame_width=-1)),
                 ("filter with u8 planes", dict(u8, **FILTER)), ("filter with u8 planes, B=0", dict(u8, **FILTER, B=0)),
                 ("workspace before filter", dict(u8, **FILTER, workspace=None)),
                 ("LDS bound", dict(BIG)), ("LDS bound, polygons", dict(poly, **BIG)), ("LDS bound, filter on", dict(BIG, **FILTER)),
                 ("workspace before LDS bound", dict(BIG, workspace=None)),
                 # behind fit_dispatch: what the instance engine refuses before its launch (the pin keeps the other engines out)
                 ("subsample mode without the bit image in LDS", dict(sample_nolds, opt_engine=INSTANCE)),
                 ("filter off with max_edge=0", dict(sample_nolds, opt_engine=INSTANCE, filter_boundary=10, filter_max_edge=0)),
                 ("filter off with boundary=-1", dict(sample_nolds, opt_engine=INSTANCE, filter_boundary=-1, filter_max_edge=10))])

    # ---- la3d_fit_instances_bits ----
    bits_v = dict(blk, mask_bits=p, bits_plane_stride=8, flags=0)
    bits_cases = (size + [("mask given", dict(mask=p)), ("rle_counts given", dict(rle_counts=p)), ("poly_xy given", dict(poly_xy=p)),
                          ("struct_size before masks", dict(struct_size=0, mask=p)),
                          ("flags=2", dict(flags=2)), ("flags=-1", dict(flags=-1)), ("masks before flags", dict(mask=p, flags=2)),
                          ("mask_bits=NULL", dict(mask_bits=None)), ("mask_bits misaligned", dict(mask_bits=p + 2)),
                          ("mask_bits=NULL, B=0", dict(mask_bits=None, B=0)), ("flags before mask_bits", dict(flags=2, mask_bits=None)),
                          ("short bits stride", dict(bits_plane_stride=7)), ("short bits stride, H=0", dict(bits_plane_stride=7, H=0)),
                          ("short bits stride, B=0", dict(bits_plane_stride=7, B=0)),
                          ("mask_bits before stride", dict(mask_bits=p + 2, bits_plane_stride=7)), ("stride before options", dict(bits_plane_stride=7, proj=p))] +
                  options + null("depth") + [("depth_plane_stride=-1", dict(depth_plane_stride=-1))] + dispatch(True) + hull_ws +
                  [("frame_width=-1", dict(frame_width=-1)), ("frame_width>W", dict(frame_width=W + 1)),
                   ("frame_width, W no multiple of 32", dict(frame_width=20, W=48, bits_plane_stride=12)),
                   ("workspace before frame_width", dict(frame_width=-1, workspace=None)),
                   ("LDS bound", dict(BIG, bits_plane_stride=1 << 16)), ("frame_width before LDS bound", dict(BIG, bits_plane_stride=1 << 16, frame_width=-1)),
                   ("workspace before LDS bound", dict(BIG, bits_plane_stride=1 << 16, workspace=None))])

    # ---- the la3d_depth16 block, as the three entries that take one check it (in two steps, the copy of the block between them) ----
    d16 = dict(d_struct_size=32, d_dtype=F16, d_planes=p, d_plane_stride=0, d_scale=1.0, d_flags=0)
    u16 = dict(d_dtype=U16, d_scale=0.001)
    d16_head = [("depth16=NULL", dict(depth16=None)), ("la3d_depth16 struct_size=31", dict(d_struct_size=31)), ("la3d_depth16 struct_size=0", dict(d_struct_size=0)),
                ("dtype=F32", dict(d_dtype=F32)), ("dtype=BF16", dict(d_dtype=BF16)), ("dtype=-1", dict(d_dtype=-1)),
                ("planes=NULL", dict(d_planes=None)), ("planes misaligned", dict(d_planes=p + 1)),
                ("struct_size before depth16=NULL", dict(struct_size=0, depth16=None)), ("args=NULL before depth16=NULL", dict(args=None, depth16=None)),
                ("la3d_depth16 struct_size before dtype", dict(d_struct_size=31, d_dtype=F32)), ("dtype before planes", dict(d_dtype=F32, d_planes=None)),
                ("planes before args->depth", dict(d_planes=None, depth=p))]
    d16_values = [("args->depth given", dict(depth=p)), ("args->depth before values", dict(depth=p, d_flags=1)),
                  ("U16 scale=0", dict(u16, d_scale=0.0)), ("U16 scale=-1", dict(u16, d_scale=-1.0)), ("U16 scale=NaN", dict(u16, d_scale=NAN)),
                  ("U16 scale=inf", dict(u16, d_scale=INF)), ("U16 flags=2", dict(u16, d_flags=2)), ("U16 flags=-1", dict(u16, d_flags=-1)),
                  ("F16 flags=1", dict(d_flags=1)), ("scale before flags", dict(u16, d_scale=0.0, d_flags=2)),
                  ("the scale of F16 planes is not read", dict(d_scale=NAN, workspace=None))]

    # ---- la3d_fit_instances_depth16 ----
    d_v = dict(blk, **rle_m, **d16, depth=None, depth16=True, mask_bits=None, bits_plane_stride=0, bits_flags=0)
    d_bits = dict(rle_counts=None, rle_offsets=None, mask_bits=p, bits_plane_stride=8)
    d_cases = (size + d16_head + d16_values +
               [("depth_plane_stride=5", dict(depth_plane_stride=5)),
                ("plane_stride=-1", dict(d_plane_stride=-1)), ("plane_stride below H*W", dict(d_plane_stride=H * W - 1)),
                ("plane_stride below H*W, H=0", dict(d_plane_stride=5, H=0)), ("values before plane_stride", dict(d_flags=1, d_plane_stride=-1)),
                ("no mask source", dict(rle_counts=None)), ("no mask source, B=0", dict(rle_counts=None, B=0)), ("two mask sources", dict(mask=p)),
                ("mask_bits and run lengths", dict(mask_bits=p, bits_plane_stride=8)), ("plane_stride before mask sources", dict(d_plane_stride=-1, mask=p)),
                ("mask sources before polygon rule", dict(poly_xy=p)),
                ("polygons without ring_offsets", dict(poly, ring_offsets=None)), ("polygons without inst_rings", dict(poly, inst_rings=None)),
                ("bits_flags=2", dict(d_bits, bits_flags=2)), ("bits_flags=-1", dict(d_bits, bits_flags=-1)),
                ("bits_flags without mask_bits are not read", dict(bits_flags=2, workspace=None)),
                ("mask_bits misaligned", dict(d_bits, mask_bits=p + 2)), ("bits_flags before mask_bits", dict(d_bits, bits_flags=2, mask_bits=p + 2)),
                ("short bits stride", dict(d_bits, bits_plane_stride=7)), ("short bits stride, B=0", dict(d_bits, bits_plane_stride=7, B=0)),
                ("mask_bits before stride", dict(d_bits, mask_bits=p + 2, bits_plane_stride=7)),
                ("stride before options", dict(d_bits, bits_plane_stride=7, proj=p)), ("polygon rule before options", dict(poly, ring_offsets=None, proj=p))] +
               options + [("rle_offsets=NULL", dict(rle_offsets=None))] + dispatch(True) + hull_ws +
               [("frame_width=-1", dict(frame_width=-1)), ("frame_width=-1, bit planes", dict(d_bits, frame_width=-1)),
                ("filter with u8 planes", dict(u8, **FILTER)),
                ("LDS bound", dict(BIG)), ("LDS bound, bit planes", dict(d_bits, **BIG, bits_plane_stride=1 << 16)),
                ("workspace before LDS bound", dict(BIG, workspace=None)),
                # behind fit_dispatch: the 16-bit units of the instance engine, each with its own copy of the rule
                ("F16: subsample mode without the bit image in LDS", dict(sample_nolds)),
                ("U16: subsample mode without the bit image in LDS", dict(sample_nolds, **u16))])

    # ---- the frames entries: what check_frames_call refuses, then the entry's own alignment rule ----
    fr = dict(frames=p, P=1)
    frames_rules = [("u8 mask planes", dict(mask=p)), ("u8 mask planes, B=0", dict(mask=p, B=0)), ("method=HULL", dict(method=HULL)),
                    ("mask before hull", dict(mask=p, method=HULL)),
                    ("no kind", dict(rle_counts=None)), ("two kinds", dict(poly_m)), ("no kind, B=0", dict(rle_counts=None, B=0)),
                    ("hull before kinds", dict(method=HULL, rle_counts=None)),
                    ("polygons without ring_offsets", dict(poly, ring_offsets=None)), ("polygons without inst_rings, B=0", dict(poly, inst_rings=None, B=0)),
                    ("kinds before polygon rule", dict(poly_xy=p))]
    frames_table = [("P=-1", dict(P=-1)), ("P=-1, B=0", dict(P=-1, B=0)), ("P=0", dict(P=0)), ("frames=NULL", dict(frames=None)),
                    ("frames misaligned", dict(frames=p + 4)), ("P=0, B=0", dict(P=0, B=0)), ("frames=NULL, B=0", dict(frames=None, B=0)),
                    ("image_index=NULL", dict(image_index=None)), ("image_index=NULL, B=0", dict(image_index=None, B=0)),
                    ("frames before image_index", dict(frames=None, image_index=None)),
                    ("depth_plane_stride=5", dict(depth_plane_stride=5)), ("frame_width=16", dict(frame_width=16)), ("frame_width=16, B=0", dict(frame_width=16, B=0)),
                    ("image_index before strides", dict(image_index=None, frame_width=16))]
    outside = [("bounds outside the tiled form", dict(WIDE)), ("bounds outside the tiled form, tall", dict(H=2048, W=32)),
               ("subsample mode: bounds outside the tiled form", dict(WIDE, sample_idx=p)),
               ("workspace before the tiled form", dict(WIDE, workspace=None)), ("bounds outside the tiled form, B=0", dict(WIDE, B=0))]
    f_v = dict(blk, **rle_m, **fr, image_index=p)
    f_cases = (size + [("struct_size before masks", dict(struct_size=0, mask=p))] + frames_rules +
               [("polygon rule before frames", dict(poly, ring_offsets=None, frames=None))] + frames_table +
               [("depth misaligned", dict(depth=p + 8)), ("depth misaligned, B=0", dict(depth=p + 8, B=0)), ("strides before depth alignment", dict(frame_width=16, depth=p + 8)),
                ("depth alignment before options", dict(depth=p + 8, opt_engine=-1))] +
               options_f + null("depth") + [("rle_offsets=NULL", dict(rle_offsets=None))] + dispatch(True) +
               [("LDS bound", dict(BIG)), ("workspace before LDS bound", dict(BIG, workspace=None))] +
               outside)

    fd_v = dict(f_v, **d16, depth=None, depth16=True)
    fd_cases = (size + d16_head + [c for c in d16_values if c[0] != "the scale of F16 planes is not read"] +
                [("plane_stride=5", dict(d_plane_stride=5)), ("values before plane_stride", dict(d_flags=1, d_plane_stride=5)),
                 ("plane_stride before masks", dict(d_plane_stride=5, mask=p))] + frames_rules + frames_table +
                [("planes not 8-byte aligned", dict(d_planes=p + 2)), ("planes not 8-byte aligned, B=0", dict(d_planes=p + 4, B=0)),
                 ("strides before planes alignment", dict(frame_width=16, d_planes=p + 2)), ("planes alignment before options", dict(d_planes=p + 2, opt_engine=-1))] +
                options_f + [("rle_offsets=NULL", dict(rle_offsets=None))] + dispatch(True) +
                [("LDS bound", dict(BIG)), ("workspace before LDS bound", dict(BIG, workspace=None))] +
                [("F16: " + n, c) for n, c in outside] + [("U16: " + n, dict(c, **u16)) for n, c in outside[:3]])

    fb_v = dict(blk, **fr, image_index=p, depth16=None, **d16, mask_bits=p, bits_offsets=p, bits_flags=0)
    with16 = dict(depth=None, depth16=True)
    fb_cases = (size + [("16-bit: " + n, dict(with16, **c)) for n, c in d16_head if "depth16=NULL" not in n] +
                [("16-bit: struct_size=0", dict(with16, struct_size=0)), ("16-bit: args=NULL", dict(with16, args=None))] +
                [("16-bit: " + n, dict(with16, **c)) for n, c in d16_values if n != "the scale of F16 planes is not read"] +
                [("16-bit: plane_stride=5", dict(with16, d_plane_stride=5)), ("16-bit: plane_stride before masks", dict(with16, d_plane_stride=5, mask=p)),
                 ("mask given", dict(mask=p)), ("rle_counts given", dict(rle_counts=p)), ("poly_xy given", dict(poly_xy=p)), ("mask given, B=0", dict(mask=p, B=0)),
                 ("struct_size before masks", dict(struct_size=0, mask=p)),
                 ("bits_flags=2", dict(bits_flags=2)), ("bits_flags=-1", dict(bits_flags=-1)), ("masks before bits_flags", dict(mask=p, bits_flags=2)),
                 ("method=HULL", dict(method=HULL)), ("bits_flags before hull", dict(bits_flags=2, method=HULL))] + frames_table +
                [("mask_bits=NULL", dict(mask_bits=None)), ("mask_bits not 16-byte aligned", dict(mask_bits=p + 8)), ("mask_bits=NULL, B=0", dict(mask_bits=None, B=0)),
                 ("strides before mask_bits", dict(frame_width=16, mask_bits=None)),
                 ("bits_offsets=NULL", dict(bits_offsets=None)), ("bits_offsets misaligned", dict(bits_offsets=p + 4)), ("bits_offsets=NULL, B=0", dict(bits_offsets=None, B=0)),
                 ("mask_bits before bits_offsets", dict(mask_bits=p + 8, bits_offsets=None)),
                 ("depth misaligned", dict(depth=p + 8)), ("depth misaligned, B=0", dict(depth=p + 8, B=0)), ("bits_offsets before depth alignment", dict(bits_offsets=None, depth=p + 8)),
                 ("16-bit: planes not 8-byte aligned", dict(with16, d_planes=p + 2)), ("16-bit: planes not 8-byte aligned, B=0", dict(with16, d_planes=p + 4, B=0)),
                 ("depth alignment before options", dict(depth=p + 8, opt_engine=-1))] +
                options_f + null("depth") + dispatch(True) + [("16-bit: " + n, dict(with16, **c)) for n, c in dispatch(True)[:3]] +
                [("LDS bound", dict(BIG)), ("workspace before LDS bound", dict(BIG, workspace=None)), ("16-bit: LDS bound", dict(with16, **BIG))] +
                outside + [("F16: " + n, dict(with16, **c)) for n, c in outside[:3]] + [("U16: " + n, dict(with16, **c, **u16)) for n, c in outside[:3]])

    # ---- la3d_fit_annotations_host: host arrays; it reads image_index and the offsets before it touches the device ----
    ah_v = dict(blk, rle_counts=host["counts"], rle_offsets=host["offsets_ok"], workspace=None)
    ah_poly = dict(rle_counts=None, rle_offsets=None, poly_xy=host["counts"], ring_offsets=host["ring_ok"], inst_rings=host["inst_ok"])
    ah_cases = (size[:3] + [("a longer block is read", dict(struct_size=FULL + 8, B=-1))] +
                [(f"{n}={v}", {n: v}) for n, v in (("B", -1), ("H", 0), ("W", 0), ("k_stride", 8))] +
                [("u8 mask planes", dict(mask=p)), ("both kinds", dict(poly_xy=host["counts"], ring_offsets=host["ring_ok"], inst_rings=host["inst_ok"])),
                 ("no kind", dict(rle_counts=None)), ("rle_offsets=NULL", dict(rle_offsets=None)),
                 ("polygons without ring_offsets", dict(ah_poly, ring_offsets=None)), ("polygons without inst_rings", dict(ah_poly, inst_rings=None))] +
                null("depth", "K", "out", "status") + [("sample_idx given", dict(sample_idx=p)), ("proj given", dict(proj=p)),
                                                       ("B=0", dict(B=0)), ("bad argument before B=0", dict(B=0, H=0)),
                                                       ("B=0 before image_index", dict(B=0, image_index=host["index_neg"])),
                                                       ("negative image_index", dict(image_index=host["index_neg"])),
                                                       ("negative run-length total", dict(rle_offsets=host["offsets_neg"])),
                                                       ("negative part total", dict(ah_poly, inst_rings=host["inst_neg"])),
                                                       ("negative vertex total", dict(ah_poly, ring_offsets=host["ring_neg"])),
                                                       ("image_index before offsets", dict(image_index=host["index_neg"], rle_offsets=host["offsets_neg"]))])

    # ---- la3d_align_ransac_batch: a block ----
    ar_v = dict(struct_size=C.sizeof(AlignRansacArgs), P=1, n=16, relative_sel=p, metric_sel=p, counts=p, min_samples=0.5, stop_probability=0.99,
                max_trials=8, m_cap=0, subsets=None, seed=1, coef=p, n_inliers=p, n_trials=p, best_trial=p, status=p, workspace=p)
    ar_ptr4 = ("relative_sel", "metric_sel", "subsets", "coef", "n_inliers", "n_trials", "best_trial", "status")
    ar_req = ("counts", "coef", "n_inliers", "n_trials", "best_trial", "status", "workspace", "relative_sel", "metric_sel")
    ar_cases = ([("args=NULL", dict(args=None)), ("struct_size=0", dict(struct_size=0)), ("a longer block", dict(struct_size=C.sizeof(AlignRansacArgs) + 8)),
                 ("P=-1", dict(P=-1)), ("n=-1", dict(n=-1)), ("struct_size before sizes", dict(struct_size=0, P=-1)),
                 ("max_trials=0", dict(max_trials=0)), ("sizes before max_trials", dict(n=-1, max_trials=0)),
                 ("min_samples=0", dict(min_samples=0.0)), ("min_samples=NaN", dict(min_samples=NAN)), ("min_samples=2.5", dict(min_samples=2.5)),
                 ("min_samples=2^31", dict(min_samples=2147483648.0)), ("max_trials before min_samples", dict(max_trials=0, min_samples=0.0)),
                 ("stop_probability=-0.1", dict(stop_probability=-0.1)), ("stop_probability=1.5", dict(stop_probability=1.5)), ("stop_probability=NaN", dict(stop_probability=NAN)),
                 ("min_samples before stop_probability", dict(min_samples=0.0, stop_probability=1.5)),
                 ("subsets with m_cap=0", dict(subsets=p)), ("stop_probability before m_cap", dict(stop_probability=1.5, subsets=p)),
                 ("m_cap before alignment", dict(subsets=p + 2))] +
                [(f"{n} misaligned", {n: p + 2, "m_cap": 4}) for n in ar_ptr4] +
                [("counts misaligned", dict(counts=p + 4)), ("workspace misaligned", dict(workspace=p + 8)),
                 ("4-byte rule before 8-byte rule", dict(coef=p + 2, counts=p + 4))] +
                [(f"{n}=NULL", {n: None}) for n in ar_req] +
                [("n=0 lets the samples be NULL", dict(n=0, relative_sel=None, metric_sel=None, max_trials=2000)),
                 ("alignment before NULL", dict(counts=p + 4, coef=None)),
                 ("too many samples", dict(n=(1 << 24) + 1)), ("too many trials", dict(max_trials=1025)), ("too many frames", dict(P=65536)),
                 ("NULL before too many samples", dict(coef=None, n=(1 << 24) + 1)), ("samples before trials", dict(n=(1 << 24) + 1, max_trials=1025)),
                 ("trials before frames", dict(max_trials=1025, P=65536)),
                 ("P=0", dict(P=0)), ("P=0, pointers NULL", dict({n: None for n in ar_req}, P=0)), ("misaligned before P=0", dict(P=0, coef=p + 2)),
                 ("too many trials before P=0", dict(P=0, max_trials=1025))])

    d16_src = dict(depth16=True, **d16)
    return {
        "la3d_fit_instances": (head + ["mask"] + cam + tail, dict(leg, mask=p),
                               leg_common + [("mask=NULL", dict(mask=None)), ("mask=NULL, B=0", dict(mask=None, B=0))]),
        "la3d_fit_instances_rle": (head + ["rle_counts", "rle_offsets"] + cam + tail, dict(leg, **rle_m), leg_common + rle_c + leg_lds),
        "la3d_fit_instances_poly": (head + ["poly_xy", "ring_offsets", "inst_rings"] + cam + tail, dict(leg, **poly_m), leg_common + poly_c + leg_lds),
        "la3d_fit_instances_rle_filtered": (head + ["rle_counts", "rle_offsets"] + cam + filt, dict(leg, **rle_m), leg_common + rle_c + leg_lds + leg_filter),
        "la3d_fit_instances_poly_filtered": (head + ["poly_xy", "ring_offsets", "inst_rings"] + cam + filt, dict(leg, **poly_m),
                                             leg_common + poly_c + leg_lds + leg_filter),
        "la3d_fit_instances_ex": (["args"], ex_v, ex_cases),
        "la3d_fit_instances_bits": (["args", "mask_bits", "bits_plane_stride", "flags"], bits_v, bits_cases),
        "la3d_fit_instances_depth16": (["args", "depth16", "mask_bits", "bits_plane_stride", "bits_flags"], d_v, d_cases),
        "la3d_fit_instances_frames": (["args", "frames", "P"], f_v, f_cases),
        "la3d_fit_instances_frames_depth16": (["args", "depth16", "frames", "P"], fd_v, fd_cases),
        "la3d_fit_instances_frames_bits": (["args", "depth16", "frames", "P", "mask_bits", "bits_offsets", "bits_flags"], fb_v, fb_cases),
        # ---- la3d_points.hip ----
        "la3d_fit_points": (["points", "offsets", "ground", "sample_idx", "method", "B", "out", "status", "aux", "stream"],
                            dict(points=p, offsets=p, ground=None, sample_idx=None, method=PCA, B=1, out=p, status=p, aux=None, stream=None),
                            [("B=-1", dict(B=-1))] + null("offsets", "out", "status", "points") +
                            [("method=2", dict(method=2)), ("method=-1", dict(method=-1)), ("hints alone are PCA", dict(method=0x300, B=0)),
                             ("a hint does not hide the method", dict(method=0x100 | 2)), ("bad argument before method", dict(B=-1, method=2)),
                             ("method before B=0", dict(method=2, B=0)), ("B=0", dict(B=0)), ("B=0, pointers NULL", dict(B=0, points=None, offsets=None, out=None, status=None))]),
        "la3d_estimate_bbox_host": (["points", "n", "ground4", "method", "out39", "aux4", "status"],
                                    dict(points=p, n=4, ground4=None, method=PCA, out39=p, aux4=None, status=p),
                                    [("n=-1", dict(n=-1)), ("n > 2^31", dict(n=(1 << 31) + 1))] + null("points", "out39", "status") +
                                    [("method=2", dict(method=2)), ("a hint is no method here", dict(method=0x100)), ("bad argument before method", dict(n=-1, method=2))]),
        "la3d_unproject_host": (["depth", "K9", "Rt12", "H", "W", "out", "out_is_f64"], dict(depth=p, K9=p, Rt12=None, H=H, W=W, out=p, out_is_f64=0),
                                null("depth", "K9", "out") + [("H=0", dict(H=0)), ("W=-1", dict(W=-1)), ("frame too large", dict(H=1 << 15, W=1 << 15))]),
        "la3d_fit_annotations_host": (["args"], ah_v, ah_cases),
        # ---- la3d_masks.hip ----
        "la3d_unproject": (["depth", "K9", "Rt12", "H", "W", "out", "out_is_f64", "stream"], dict(depth=p, K9=p, Rt12=None, H=H, W=W, out=p, out_is_f64=0, stream=None),
                           null("depth", "K9", "out") + [("H=0", dict(H=0)), ("W=-1", dict(W=-1)), ("frame too large", dict(H=1 << 15, W=1 << 15))]),
        "la3d_unproject_batch": (["depth", "K", "k_stride", "Rt12", "P", "H", "W", "out", "out_is_f64", "stream"],
                                 dict(depth=p, K=p, k_stride=0, Rt12=None, P=1, H=H, W=W, out=p, out_is_f64=0, stream=None),
                                 null("depth", "K", "out") + [("P=-1", dict(P=-1)), ("P=65536", dict(P=65536)), ("H=0", dict(H=0)), ("W=-1", dict(W=-1)),
                                                              ("frame too large", dict(H=1 << 15, W=1 << 15)), ("k_stride=8", dict(k_stride=8)), ("k_stride=-9", dict(k_stride=-9)),
                                                              ("P=0", dict(P=0)), ("bad argument before P=0", dict(P=0, out=None))]),
        "la3d_pad_rows": (["src", "rows", "W", "Wp", "dst", "stream"], dict(src=p, rows=4, W=30, Wp=32, dst=p, stream=None),
                          [("rows=-1", dict(rows=-1)), ("W=0", dict(W=0)), ("Wp<W", dict(Wp=28)), ("Wp no multiple of 4", dict(Wp=34))] + null("src", "dst") +
                          [("dst misaligned", dict(dst=p + 8)), ("rows=0", dict(rows=0)), ("rows=0, pointers NULL", dict(rows=0, src=None, dst=None)),
                           ("dst misaligned, rows=0", dict(rows=0, dst=p + 8))]),
        "la3d_mask_counts": (["mask", "B", "H", "W", "counts", "stream"], dict(mask=p, B=1, H=H, W=W, counts=p, stream=None),
                             null("mask", "counts") + [("B=-1", dict(B=-1)), ("H=0", dict(H=0)), ("W=0", dict(W=0)), ("B=0", dict(B=0)), ("mask=NULL, B=0", dict(mask=None, B=0))]),
        "la3d_mask_stats_poly": (["poly_xy", "ring_offsets", "inst_rings", "B", "H", "W", "boundary", "stats", "stream"],
                                 dict(poly_xy=p, ring_offsets=p, inst_rings=p, B=1, H=H, W=W, boundary=1, stats=p, stream=None),
                                 null("poly_xy", "ring_offsets", "inst_rings", "stats") +
                                 [("B=-1", dict(B=-1)), ("H=0", dict(H=0)), ("W=0", dict(W=0)), ("boundary=-1", dict(boundary=-1)), ("H*W > 2^20", dict(BIG)),
                                  ("H*W > 2^20 before B=0", dict(BIG, B=0)), ("B=0", dict(B=0)), ("B=0, pointers NULL", dict(B=0, poly_xy=None, ring_offsets=None, inst_rings=None, stats=None)),
                                  ("too many rows for LDS", dict(H=1 << 20, W=1)), ("B=0 before too many rows", dict(H=1 << 20, W=1, B=0)),
                                  ("bad argument before too many rows", dict(H=1 << 20, W=1, boundary=-1))]),
        "la3d_mask_stats": (["mask", "B", "H", "W", "boundary", "stats", "stream"], dict(mask=p, B=1, H=H, W=W, boundary=1, stats=p, stream=None),
                            null("mask", "stats") + [("B=-1", dict(B=-1)), ("H=0", dict(H=0)), ("W=0", dict(W=0)), ("boundary=-1", dict(boundary=-1)),
                                                     ("B=0", dict(B=0)), ("mask=NULL, B=0", dict(mask=None, B=0))]),
        "la3d_mask_stats_rle": (["counts", "offsets", "B", "H", "W", "boundary", "stats", "stream"],
                                dict(counts=p, offsets=p, B=1, H=H, W=W, boundary=1, stats=p, stream=None),
                                null("counts", "offsets", "stats") +
                                [("B=-1", dict(B=-1)), ("H=0", dict(H=0)), ("W=0", dict(W=0)), ("boundary=-1", dict(boundary=-1)), ("H=32769", dict(H=32769)),
                                 ("H*W > 2^30", dict(H=32768, W=32769)), ("B=0", dict(B=0)), ("counts=NULL, B=0", dict(counts=None, B=0)),
                                 ("offsets=NULL, B=0", dict(offsets=None, B=0))]),
        # ---- la3d_consumers.hip ----
        "la3d_masked_ratio_median": (["num", "num_plane_stride", "image_index", "den", "mask_a", "mask_b", "B", "H", "W", "median", "count", "stream"],
                                     dict(num=p, num_plane_stride=0, image_index=None, den=p, mask_a=p, mask_b=None, B=1, H=H, W=W, median=p, count=p, stream=None),
                                     null("num", "den", "mask_a", "median", "count") +
                                     [("B=-1", dict(B=-1)), ("H=0", dict(H=0)), ("W=0", dict(W=0)), ("num_plane_stride=-1", dict(num_plane_stride=-1)),
                                      ("B=0", dict(B=0)), ("num=NULL, B=0", dict(num=None, B=0)), ("frame too large for LDS", dict(H=1024, W=1024)),
                                      ("B=0 before too large", dict(H=1024, W=1024, B=0)), ("bad argument before too large", dict(H=1024, W=1024, count=None))]),
        "la3d_align_select_batch": (["relative", "metric", "mask", "P", "n", "max_valid_depth", "relative_out", "metric_out", "counts", "workspace", "stream"],
                                    dict(relative=p, metric=p, mask=None, P=1, n=16, max_valid_depth=10.0, relative_out=p, metric_out=p, counts=p, workspace=p, stream=None),
                                    [("P=-1", dict(P=-1)), ("P=65536", dict(P=65536)), ("n=-1", dict(n=-1))] +
                                    null("counts", "workspace", "relative", "metric", "relative_out", "metric_out") +
                                    [("P=0", dict(P=0)), ("P=0, pointers NULL", dict(P=0, counts=None, workspace=None, relative=None)), ("n=-1 before P=0", dict(P=0, n=-1))]),
        "la3d_align_select": (["relative", "metric", "mask", "n", "max_valid_depth", "relative_out", "metric_out", "count", "workspace", "stream"],
                              dict(relative=p, metric=p, mask=None, n=16, max_valid_depth=10.0, relative_out=p, metric_out=p, count=p, workspace=p, stream=None),
                              [("n=-1", dict(n=-1))] + null("count", "workspace", "relative", "metric", "relative_out", "metric_out") +
                              [("count=NULL, n=0", dict(count=None, n=0))]),
        "la3d_align_apply": (["relative", "mask", "n", "coef", "intercept", "fill", "out", "stream"],
                             dict(relative=p, mask=None, n=16, coef=1.0, intercept=0.0, fill=0.0, out=p, stream=None),
                             [("n=-1", dict(n=-1))] + null("relative", "out") + [("n=0", dict(n=0)), ("n=0, pointers NULL", dict(n=0, relative=None, out=None))]),
        "la3d_unproject_matches": (["depth", "H", "W", "uv", "N", "fx", "fy", "cx", "cy", "use_flip", "flip", "R9", "T3", "out", "valid", "stream"],
                                   dict(depth=p, H=H, W=W, uv=p, N=4, fx=100.0, fy=100.0, cx=16.0, cy=4.0, use_flip=0, flip=0.0, R9=None, T3=None, out=p, valid=p, stream=None),
                                   null("depth", "uv", "out", "valid") +
                                   [("N=-1", dict(N=-1)), ("H=0", dict(H=0)), ("W=0", dict(W=0)), ("R9 without T3", dict(R9=p)), ("T3 without R9", dict(T3=p)),
                                    ("N=0", dict(N=0)), ("uv=NULL, N=0", dict(uv=None, N=0)), ("out=NULL, N=0", dict(out=None, N=0))]),
        "la3d_project_boxes": (["records", "K", "k_stride", "image_index", "B", "width", "height", "out", "stream"],
                               dict(records=p, K=p, k_stride=0, image_index=None, B=1, width=640.0, height=480.0, out=p, stream=None),
                               null("records", "K", "out") + [("B=-1", dict(B=-1)), ("k_stride=8", dict(k_stride=8)), ("k_stride=-9", dict(k_stride=-9)),
                                                              ("B=0", dict(B=0)), ("records=NULL, B=0", dict(records=None, B=0)), ("K=NULL, B=0", dict(K=None, B=0))]),
        "la3d_iou_matrix": (["boxes_a", "na", "boxes_b", "nb", "out", "stream"], dict(boxes_a=p, na=2, boxes_b=p, nb=3, out=p, stream=None),
                            [("na=-1", dict(na=-1)), ("nb=-1", dict(nb=-1))] + null("boxes_a", "boxes_b", "out") +
                            [("na=0", dict(na=0)), ("nb=0", dict(nb=0)), ("na=0, pointers NULL", dict(na=0, boxes_a=None, boxes_b=None, out=None)),
                             ("nb=-1 before na=0", dict(na=0, nb=-1))]),
        # ---- la3d_depth16.hip ----
        "la3d_pack_depth16": (["depth", "plane_stride", "P", "H", "W", "W_out", "dtype", "scale", "out", "out_plane_stride", "stream"],
                              dict(depth=p, plane_stride=H * W, P=2, H=H, W=W, W_out=W, dtype=F16, scale=1.0, out=p, out_plane_stride=H * W, stream=None),
                              [("dtype=F32", dict(dtype=F32)), ("dtype=BF16", dict(dtype=BF16)), ("dtype=-1", dict(dtype=-1)), ("dtype before sizes", dict(dtype=F32, H=0)),
                               ("U16 scale=0", dict(dtype=U16, scale=0.0)), ("U16 scale=NaN", dict(dtype=U16, scale=NAN)), ("U16 scale=inf", dict(dtype=U16, scale=INF)),
                               ("the scale of F16 planes is not read", dict(scale=NAN, H=0)), ("scale before sizes", dict(dtype=U16, scale=0.0, H=0)),
                               ("P=-1", dict(P=-1)), ("H=0", dict(H=0)), ("W=0", dict(W=0)), ("W_out<W", dict(W_out=W - 1)), ("frame too large", dict(H=1 << 15, W=1 << 14, W_out=1 << 14)),
                               ("plane_stride=-1", dict(plane_stride=-1, P=1))] + null("depth", "out") +
                              [("depth misaligned", dict(depth=p + 2)), ("out misaligned", dict(out=p + 1)), ("short plane_stride", dict(plane_stride=H * W - 1)),
                               ("short out_plane_stride", dict(out_plane_stride=H * W - 1)), ("P=0", dict(P=0)), ("P=0, pointers NULL", dict(P=0, depth=None, out=None)),
                               ("P=0, short strides", dict(P=0, plane_stride=0, out_plane_stride=0)), ("sizes before P=0", dict(P=0, W_out=W - 1)),
                               ("scale before P=0", dict(P=0, dtype=U16, scale=0.0))]),
        "la3d_unpack_depth16": (["depth16", "P", "H", "W_in", "W", "out", "stream"], dict(d16_src, d_plane_stride=H * W, P=2, H=H, W_in=W, W=W, out=p, stream=None),
                                [("src=NULL", dict(depth16=None)), ("struct_size=31", dict(d_struct_size=31)), ("struct_size=0", dict(d_struct_size=0)),
                                 ("dtype=F32", dict(d_dtype=F32)), ("dtype=BF16", dict(d_dtype=BF16)), ("struct_size before dtype", dict(d_struct_size=31, d_dtype=F32)),
                                 ("U16 scale=0", dict(u16, d_scale=0.0)), ("U16 scale=NaN", dict(u16, d_scale=NAN)), ("U16 scale=inf", dict(u16, d_scale=INF)),
                                 ("U16 flags=2", dict(u16, d_flags=2)), ("F16 flags=1", dict(d_flags=1)), ("dtype before values", dict(d_dtype=F32, d_flags=1)),
                                 ("values before sizes", dict(d_flags=1, H=0)),
                                 ("P=-1", dict(P=-1)), ("H=0", dict(H=0)), ("W=0", dict(W=0)), ("W_in<W", dict(W_in=W - 1)), ("frame too large", dict(H=1 << 15, W_in=1 << 14, W=1 << 14)),
                                 ("plane_stride=-1", dict(d_plane_stride=-1)), ("planes=NULL", dict(d_planes=None)), ("out=NULL", dict(out=None)),
                                 ("planes misaligned", dict(d_planes=p + 1)), ("short plane_stride", dict(d_plane_stride=H * W - 1)),
                                 ("P=0", dict(P=0)), ("P=0, pointers NULL", dict(P=0, d_planes=None, out=None)), ("sizes before P=0", dict(P=0, W_in=W - 1)),
                                 ("values before P=0", dict(P=0, d_flags=1))]),
        # ---- la3d_align.hip ----
        "la3d_align_ransac_batch": (["args"], ar_v, ar_cases),
        "la3d_align_ransac_subsets": (["counts", "P", "min_samples", "max_trials", "seed", "subsets", "m_cap", "stream"],
                                      dict(counts=p, P=1, min_samples=0.5, max_trials=8, seed=1, subsets=p, m_cap=4, stream=None),
                                      [("P=-1", dict(P=-1)), ("max_trials=0", dict(max_trials=0)), ("m_cap=0", dict(m_cap=0)), ("min_samples=0", dict(min_samples=0.0)),
                                       ("min_samples=NaN", dict(min_samples=NAN)), ("min_samples=2.5", dict(min_samples=2.5)), ("min_samples=2^31", dict(min_samples=2147483648.0))] +
                                      null("counts", "subsets") +
                                      [("counts misaligned", dict(counts=p + 4)), ("subsets misaligned", dict(subsets=p + 2)),
                                       ("too many trials", dict(max_trials=1025)), ("too many frames", dict(P=65536)), ("bad argument before too many trials", dict(max_trials=1025, m_cap=0)),
                                       ("P=0", dict(P=0)), ("P=0, pointers NULL", dict(P=0, counts=None, subsets=None)), ("misaligned before P=0", dict(P=0, subsets=p + 2)),
                                       ("too many trials before P=0", dict(P=0, max_trials=1025))]),
        "la3d_align_apply_batch": (["relative", "metric", "mask", "P", "n", "coef", "status", "fill", "out", "stream"],
                                   dict(relative=p, metric=p, mask=None, P=1, n=16, coef=p, status=p, fill=0.0, out=p, stream=None),
                                   [("P=-1", dict(P=-1)), ("P=65536", dict(P=65536)), ("n=-1", dict(n=-1))] + null("relative", "metric", "coef", "status", "out") +
                                   [(f"{n} misaligned", {n: p + 2}) for n in ("relative", "metric", "coef", "status", "out")] +
                                   [("P=0", dict(P=0)), ("n=0", dict(n=0)), ("n=0, pointers NULL", dict(n=0, relative=None, metric=None, coef=None, status=None, out=None)),
                                    ("misaligned before P=0", dict(P=0, out=p + 2)), ("frame too large", dict(n=1 << 40)), ("P=0 before too large", dict(P=0, n=1 << 40)),
                                    ("bad argument before too large", dict(n=1 << 40, out=None))]),
    }


def _host_arrays():
    """the arrays la3d_fit_annotations_host reads; ring_* / inst_* are addressed one element in, so that index -1 is still the array's"""
    i64, i32 = C.c_int64, C.c_int32
    arrays = dict(counts=(i32 * 8)(0, 4, 0, 0, 0, 0, 0, 0), index_neg=(i32 * 2)(-1, 0), offsets_ok=(i64 * 2)(0, 2), offsets_neg=(i64 * 2)(0, -1),
                  ring_ok=(i64 * 3)(0, 0, 4), ring_neg=(i64 * 3)(0, 0, -5), inst_ok=(i64 * 3)(0, 0, 1), inst_neg=(i64 * 3)(0, 0, -1))
    addr = {k: C.addressof(v) + (8 if k.startswith(("ring_", "inst_")) else 0) for k, v in arrays.items()}
    return arrays, addr


def _call(lib, entry, order, a, block_type):
    from labelany3d_amd._lib import Depth16Block

    fn = getattr(lib, entry)
    argv, keep = [], []
    for name, ctype in zip(order, fn.argtypes):
        if name == "args":
            if "args" in a and a["args"] is None:
                argv.append(None)
                continue
            block = block_type(**{f: a[f] for f, _ in block_type._fields_ if f in a})      # (the stream stays NULL)
            keep.append(block)
            argv.append(C.byref(block))
        elif name == "depth16":
            if a["depth16"] is None:
                argv.append(None)
                continue
            block = Depth16Block(struct_size=a["d_struct_size"], dtype=a["d_dtype"], planes=a["d_planes"], plane_stride=a["d_plane_stride"],
                                 scale=a["d_scale"], flags=a["d_flags"])
            keep.append(block)
            argv.append(C.byref(block))
        elif isinstance(a[name], int) and hasattr(ctype, "contents"):      # a typed pointer parameter (const double*)
            argv.append(C.cast(C.c_void_p(a[name]), ctype))
        else:
            argv.append(a[name])
    assert len(argv) == len(fn.argtypes), entry
    return fn(*argv)


def run(lib):
    buf = (C.c_double * 64)()
    p = (C.addressof(buf) + 15) & ~15
    arrays, host = _host_arrays()
    blocks = _blocks()
    out = []
    for entry, (order, valid, cases) in specs(p, host).items():
        block_type = blocks.get(entry)
        known = set(order) | set(valid) | ({f for f, _ in block_type._fields_} if block_type else set())
        names = [n for n, _ in cases]
        assert len(names) == len(set(names)), (entry, [n for n in names if names.count(n) > 1])
        for name, change in cases:
            assert set(change) <= known, (entry, name)
            rc = _call(lib, entry, order, dict(valid, **change), block_type)
            out.append([entry, name, rc, lib.la3d_last_error().decode() if rc != 0 else ""])
    del arrays
    return out


if __name__ == "__main__":      # python -m tests.entry_refusal_cases FILE: record FILE from the library that labelany3d_amd loads
    import json
    import sys

    from labelany3d_amd import _lib

    head = {"recorded_from": "the library of commit 3267327 (the commit before refuse(); see tests/test_entry_refusals_contract.py)",
            "format": "[entry, case, return code, la3d_last_error() or '' for a success]"}
    with open(sys.argv[1], "w") as f:
        f.write("{\n" + "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in head.items()) + ' "cases": [\n' +
                ",\n".join("  " + json.dumps(r) for r in run(_lib.lib)) + "\n ]\n}\n")
