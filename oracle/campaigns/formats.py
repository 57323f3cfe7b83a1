"""The randomised differential campaign over the format converters in front of the fit: the mask, logit and label packers
(pack_bits_vec_kernel / pack_bits_kernel, pack_labels_vec_kernel / pack_labels_kernel, pack_labels_frames_vec_kernel /
pack_labels_frames_rgb8_kernel, pack_masks_frames_kernel, unpack_mask_bits_kernel, mask_stats_bits_kernel: labelany3d_amd/csrc/
la3d_bits.hip) and the 16-bit depth packers (pack_depth16_kernel / unpack_depth16_kernel: la3d_depth16.hip) - case generator, oracle,
GPU runs and the checker.  profiles/formats/fuzz_formats.py drives it at scale; tests/test_gpu_differential.py runs a committed slice of
its seeds (tests/campaign_slices.py::FORMAT_SEEDS).

One CASE = P images, each with its own size, a label map (u8 / u16 / int16 read as uint16 / int32 / rgb8) with the ids asked of it, a
stack of instance masks (u8 bytes or bool) with the logits that mean a stack of their own (float32 / float16 / bfloat16, generated as
BIT PATTERNS of the stored type, so nothing depends on a conversion under test), a float32 depth plane and one camera.  In about half
of the cases all images share one size: the uniform entries (pack_mask_bits, pack_logits_bits, pack_label_bits, unpack_mask_bits,
mask_stats_bits, fit_instances_bits) apply to those only, the frames entries (pack_mask_bits_frames, pack_label_bits_frames,
fit_instances_frames_bits) and the depth packers to every case.  The frames are the smallest at which a stated path is entered:
  tiny, odd frames  1x1, 1x333, 1000x1, 5x13, 7x45, 8x32, 33x47, 50x75, 64x96, 96x224, 100x214; at most one 480x640 image per case
  vector packer     plane_chunks caps a plane at CHUNKS = 64 workgroups of 256 lanes, one 16-byte group each, so the g0 loop of
                    pack_bits_vec_kernel takes a second trip above 16384 groups: 129x512 (f32, 4 elements per group), 258x512
                    (f16 / bf16, 8) and 516x512 (u8, 16) have 16512 groups - one full trip and a partial one, whose DPP OR runs with
                    lanes beyond the plane; B <= 2, frame_pad=False, an aligned base
  general packer    pack_bits_kernel gives one lane a word: 1031x509 with frame_pad=False (16400 words, a ragged last one) and
                    1025x500 padded to 512 (16400 words) take its second trip; B <= 2
  unpacker          hand-made MaskBits stored (W_in, frame_width) = (53, 52), (54, 52), (37, 36) - the quad form whose shift passes 28
                    and reads two words - next to (64, 64) (quad, one word) and (64, 53) (byte form); 129x512: the second trip of the
                    quad form (16512 quads).  An unaligned `mask` base cannot be produced through the Python entry, which allocates
                    its own output: it is not run
  depth, long       4194560x1 (P = 1): grid_for caps the grid at GRID = 16384 workgroups of 256, so both depth kernels loop again above
                    4194304 groups of 8 output pixels (one per row of a 1-column frame) / pixels
The second-trip, unpacker and long frames are PACKER-ONLY (c["packer_only"]): packers, unpacker and statistics, never a fit.
  u8 bytes          1, 0xff, or a random one of 1 / 2 / 0x80 / 0xff per pixel; bool masks
  labels            the ends of every dtype's range, negative int16 / int32 ids, ids on all three bytes of rgb8; asked ids include
                    absent ids, repeated ids, images without ids and ids outside the dtype's range (tests/test_gpu_labels.py::OUTSIDE)
  logits            thresholds THRESHOLDS (0.1, 1/3, 1e-6, 7e4 are not representable in float16 / bfloat16; float(threshold) is rounded
                    to float32 at the C boundary); the stored values adjacent to the float32 threshold (neighbours: the largest <= it,
                    the smallest > it), +-0, subnormals, the largest finite value, +-inf, NaNs of both signs with payloads; the rest is
                    the mask's meaning, a few steps of the stored type either side of the threshold
  layouts           host arrays; device tensors read in place (plane stride above H*W, also one that is no multiple of 16 bytes, a base 1,
                    5 or 16 elements into an allocation); for the frames mask packer canvas crops whose pitch is / is not a multiple of
                    16 bytes, a lowest data_ptr() that is not the first image's, a (0, H, W) stack, rows in shuffled image_index order;
                    host and device ids for both label packers; out= buffers filled with SENT, wider than the planes
  16-bit depth      planes of engines.one_plane (NaN, +-inf, 0, negative pixels) with - for u16 - exact ties (k + 0.5) * scale at the
                    power-of-two scales 2^-10 and 2^-8 for even and odd k, the floats next to a tie, values at and above 65535 units
                    and float32 subnormals planted; scales clouds.SCALES plus the two powers of two; quantise / upconvert are clouds'
  broken inputs     of the frames mask packer (about one case in eight): a negative src_offsets entry or a pitch below frame_width -
                    an all-zero plane, area 0 -; an image_index outside the table or a bits_offsets entry that is negative or no
                    multiple of 4 - an untouched plane, area 0

expected(c) is plain NumPy: the meant masks (bytes != 0; labels == id after zero extension, rgb R + 256 G + 65536 B; logit patterns
up-converted exactly - astype for float16, pattern << 16 for bfloat16 - and compared > np.float32(threshold)), their areas, O.mask_stats,
quantise / upconvert, and the oracle's fit of the meant masks.  check_run lays them out (np.packbits, LSB first, rows zero-padded to the
stored width; frames.frame_bits_offsets or the uniform stride of device ids) and holds every run to RULES, each exact, no waiver:
words, padding, area, layout, sentinel, roundtrip, stats (boundary 10 and 3), depth16, agree (the decoded planes of every run equal
its family's first run), fit (status / n_masked / n_valid exact, records by tests/test_gpu_parity.py::assert_records with
reference_axis_noise as engines.check_run applies it; a reported eigen-gap below 1e-9 is the documented don't-care - counted, held to
status and counts - only where the oracle's own gap is below 1e-6 too: anything else is a wrong gap and fails).
Left out on purpose: graph capture and streams (the hand tests have them); an overread behind the last column of a dense plane (not
observable without a fault); frames so large that only the host time grows.

The oracle is test infrastructure: it is the checker here."""
import numpy as np

from .clouds import SCALES, quantise, upconvert

LANES = 256            # lanes of a workgroup of every packer
CHUNKS = 64            # plane_chunks: workgroups per plane (la3d_bits.hip)
GROUP_BYTES = 16       # pack_bits_vec_kernel: bytes a lane loads
GRID = 16384           # grid_for: workgroups of the depth packers (la3d_depth16.hip)
DEPTH_GROUP = 8        # pack_depth16_kernel: output pixels of a lane
SENT = 0x5A5A5A5A      # what an out= buffer holds before the call
SENT16 = 0x5A5A
ELEM_BYTES = {"u8": 1, "f16": 2, "bf16": 2, "f32": 4}

TINY = [(1, 1), (1, 333), (1000, 1), (5, 13), (7, 45), (8, 32), (33, 47), (50, 75), (64, 96), (96, 224), (100, 214)]
BIG = (480, 640)
VEC2 = {(129, 512): "f32", (258, 512): "f16", (516, 512): "u8"}          # frame -> the widest element that takes the second trip
GEN2 = [(1031, 509), (1025, 500)]
UNPACK = [(53, 52), (54, 52), (37, 36), (64, 64), (64, 53)]               # (W_in, frame_width) of hand-made MaskBits
LONG = (4194560, 1)
THRESHOLDS = [0.0, -0.0, 0.5, -1.25, 0.1, 1.0 / 3.0, 1e-6, 65504.0, 7e4]
LOGIT_TYPES = ("f32", "f16", "bf16")
LABEL_TYPES = ("u8", "u16", "i16", "i32", "rgb8")
D16_SCALES = SCALES + [2.0 ** -10, 2.0 ** -8]
BROKEN = ("src_offsets < 0", "pitch < frame_width", "image_index outside", "bits_offsets < 0", "bits_offsets % 4")
FAMILIES = ("masks", "logits", "labels")


# ------------------------------------------------------------------------------------------------------------------------------
# the limits of the kernels, restated
# ------------------------------------------------------------------------------------------------------------------------------
def padded_width(W):
    return (W + 31) // 32 * 32


def trips(items):
    """Trips of a plane's grid-stride loop over `items` lanes' worth of work: plane_chunks workgroups of LANES, at most CHUNKS."""
    chunks = min(max(-(-items // LANES), 1), CHUNKS)
    return -(-items // (chunks * LANES))


def vec_form(H, W, W_out, elem, base_bytes=0, stride_elems=None):
    """pack_bits_launch: the vector form needs unpadded rows, whole words and 16-byte aligned planes."""
    es = ELEM_BYTES[elem]
    stride = H * W if stride_elems is None else stride_elems
    return W_out == W and (H * W) % 32 == 0 and base_bytes % 16 == 0 and (stride * es) % 16 == 0


def pack_trips(H, W, W_out, elem):
    """Trips of the packer a dense, aligned plane takes."""
    if vec_form(H, W, W_out, elem):
        return trips(H * W // (GROUP_BYTES // ELEM_BYTES[elem]))
    return trips((H * W_out + 31) // 32)


def unpack_trips(H, W):
    """unpack_mask_bits_kernel on a 4-byte aligned output: quads where W % 4 == 0."""
    return trips(H * W // 4 if W % 4 == 0 else H * W)


def depth_trips(P, H, W, W_out):
    """(pack_depth16_kernel, unpack_depth16_kernel) trips."""
    grid = lambda n: min(max(-(-n // LANES), 1), GRID)   # noqa: E731
    g, n = P * H * ((W_out + DEPTH_GROUP - 1) // DEPTH_GROUP), P * H * W
    return -(-g // (grid(g) * LANES)), -(-n // (grid(n) * LANES))


def bits_offsets(sizes, image_index):
    """frames.frame_bits_offsets, restated: row b holds H * pitch / 32 words, every start rounded up to 4 words."""
    words = np.asarray([h * padded_width(w) // 32 for h, w in sizes], np.int64)[np.asarray(image_index, np.int64)]
    step = (words + 3) // 4 * 4
    return np.concatenate([[0], np.cumsum(step)[:-1]]).astype(np.int64) if len(step) else np.zeros(0, np.int64), int(step.sum())


# ------------------------------------------------------------------------------------------------------------------------------
# logits as bit patterns
# ------------------------------------------------------------------------------------------------------------------------------
def _bits(T):
    return 32 if T == "f32" else 16


def to_f32(pat, T):
    """The exact float32 value of stored patterns."""
    pat = np.asarray(pat)
    if T == "f32":
        return pat.astype(np.uint32).view(np.float32)
    if T == "f16":
        return pat.astype(np.uint16).view(np.float16).astype(np.float32)
    return (pat.astype(np.uint32) << 16).view(np.float32)


def key_of(pat, T):
    """A pattern's place in value order (int64): ... -min < -0 (-1) < +0 (0) < +min ... ; adjacent keys are adjacent values."""
    b = _bits(T)
    pat = np.asarray(pat).astype(np.int64)
    mag = pat & ((1 << (b - 1)) - 1)
    return np.where(pat >> (b - 1), -mag - 1, mag)


def pat_of(key, T):
    b = _bits(T)
    key = np.asarray(key, np.int64)
    return np.where(key >= 0, key, (1 << (b - 1)) | (-key - 1)).astype(np.uint32 if b == 32 else np.uint16)


def key_inf(T):
    return {"f32": 0x7F800000, "f16": 0x7C00, "bf16": 0x7F80}[T]


def neighbours(t, T):
    """(the largest stored value <= float32(t), the smallest > it) as patterns: adjacent keys."""
    t32 = np.float32(t)
    if T == "f32":
        le = int(key_of(t32.view(np.uint32), T))
        le = 0 if le == -1 else le                          # (-0.0 == +0.0: the larger key)
    else:
        allp = np.arange(65536, dtype=np.uint32)
        v = to_f32(allp, T)
        with np.errstate(invalid="ignore"):
            ok = v <= t32
        le = int(key_of(allp[ok], T).max())
    return pat_of(le, T)[()], pat_of(le + 1, T)[()]


def specials(T):
    """Patterns sprinkled in whatever the mask says: +-0, subnormals, the largest finite value, +-inf, NaNs with sign and payload."""
    b, ki = _bits(T), key_inf(T)
    sign = 1 << (b - 1)
    minnorm = {"f32": 0x00800000, "f16": 0x0400, "bf16": 0x0080}[T]
    pats = [0, sign, 1, sign | 1, minnorm - 1, sign | (minnorm - 1), minnorm, ki - 1, sign | (ki - 1), ki, sign | ki,
            ki + 1, sign | (ki + 1), ki | (minnorm >> 1) | 5, sign | ki | (minnorm >> 1) | 0x2A, sign | ((1 << (b - 1)) - 1)]
    return np.asarray(pats, np.uint32 if b == 32 else np.uint16)


def logit_planes(rs, stack, t, T):
    """Patterns of type T that mean the bool stack under `x > float32(t)`, except where a special value is sprinkled in."""
    le, gt = neighbours(t, T)
    kle, ki = int(key_of(le, T)), key_inf(T)
    steps = np.asarray([0, 1, 2, 17, 1000, 40000 if T != "f32" else 1 << 24])
    d = steps[rs.randint(0, len(steps), stack.shape)]
    key = np.where(stack, np.minimum(kle + 1 + d, ki), np.maximum(kle - d, -ki - 1))
    pat = pat_of(key, T)
    sp = np.concatenate([specials(T), np.asarray([le, gt], pat.dtype)])
    hit = rs.rand(*stack.shape) < 0.12
    pat[hit] = sp[rs.randint(0, len(sp), int(hit.sum()))]
    return pat


def logit_mask(pat, t, T):
    with np.errstate(invalid="ignore"):
        return to_f32(pat, T) > np.float32(t)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
def label_values(maps, dtype):
    """Stored label maps -> the ids they hold after zero extension (int64)."""
    a = np.asarray(maps)
    if dtype == "rgb8":
        a = a.astype(np.int64)
        return a[..., 0] | (a[..., 1] << 8) | (a[..., 2] << 16)
    if dtype in ("u8", "u16"):
        return a.astype(np.int64)
    if dtype == "i16":
        return a.view(np.uint16).astype(np.int64)
    return a.astype(np.int64)


def _encode_labels(values, dtype):
    if dtype == "u8":
        return values.astype(np.uint8)
    if dtype == "u16":
        return values.astype(np.uint16)
    if dtype == "i16":
        return values.astype(np.uint16).view(np.int16)
    if dtype == "i32":
        return values.astype(np.int32)
    return np.stack([values & 255, (values >> 8) & 255, (values >> 16) & 255], -1).astype(np.uint8)


def _palette(rs, dtype, n):
    from tests.test_gpu_labels import ENDS, RANGE

    kind = "u16" if dtype == "i16" else dtype
    lo, hi = RANGE[kind]
    ids = list(ENDS[kind]) + ([0x8000, 0xFFFE] if dtype == "i16" else [])
    while len(ids) < n:
        v = int(rs.randint(lo, hi, dtype=np.int64))
        if v not in ids:
            ids.append(v)
    return np.asarray(ids, np.int64)[rs.permutation(len(ids))[:n]]


def draw_frames(rs):
    """-> (sizes, uniform, class, w_in: the stored width of the hand-made MaskBits or None)"""
    u = rs.rand()
    if u < 0.09:
        return [list(VEC2)[rs.randint(3)]], True, "vec2", None
    if u < 0.15:
        return [GEN2[rs.randint(2)]], True, "gen2", None
    if u < 0.25:
        w_in, fw = UNPACK[rs.randint(len(UNPACK))]
        return [(int(rs.randint(3, 41)), fw)], True, "unpack", w_in
    if u < 0.28:
        return [LONG], True, "long", None
    if rs.rand() < 0.5:
        size = BIG if rs.rand() < 0.1 else TINY[rs.randint(len(TINY))]
        return [size] * (1 if size == BIG else int(rs.randint(1, 4))), True, "tiny", None
    P = int(rs.randint(3, 7))
    sizes = [TINY[i] for i in rs.choice(len(TINY), P, replace=False)]
    if rs.rand() < 0.15:
        sizes[rs.randint(P)] = BIG
    return sizes, False, "tiny", None


def plant_depth(rs, d, scale):
    """u16 edge values in a few pixels of a float32 plane: ties at (k + 0.5) * scale for even and odd k, the floats next to them,
    65535 units and beyond, float32 subnormals -> names of what was planted"""
    f = d.reshape(-1)
    s = np.float32(scale)
    k = rs.randint(1, 60000, 4).astype(np.float32)
    k[0], k[1] = np.float32(2 * rs.randint(1, 30000)), np.float32(2 * rs.randint(1, 30000) + 1)
    ties = (k + np.float32(0.5)) * s
    vals = [ties[0], ties[1], np.nextafter(ties[2], np.float32(0)), np.nextafter(ties[3], np.float32(np.inf)), np.float32(65535) * s,
            np.float32(65535.5) * s, np.float32(65536) * s, np.float32(1e-45), np.float32(1e-39), np.float32(0.5) * s, np.float32(0.49) * s]
    names = ["tie, even k", "tie, odd k", "below a tie", "above a tie", "65535 units", "65535.5 units", "above 65535 units", "subnormal", "subnormal",
             "half a unit", "below half a unit"]
    n = min(len(vals), max(1, f.size // 16))
    pick = rs.permutation(len(vals))[:n]
    at = rs.choice(f.size, n, replace=False)
    f[at] = np.asarray(vals, np.float32)[pick]
    exact = float(np.log2(scale)).is_integer()
    return {names[i] + (" (power-of-two scale)" if exact and "tie" in names[i] else "") for i in pick}


def make_case(seed):
    """One case of the campaign (inputs only), deterministic from the seed."""
    from tests.test_gpu_labels import OUTSIDE, blocky

    from . import engines as E

    rs = np.random.RandomState(seed)
    sizes, uniform, fclass, w_in = draw_frames(rs)
    P = len(sizes)
    packer_only = fclass != "tiny"
    long = fclass == "long"
    small_b = fclass in ("vec2", "gen2")
    none = int(rs.randint(P)) if P > 2 else None                 # the image without masks and without ids
    scale = D16_SCALES[rs.randint(len(D16_SCALES))]
    depth, planted = [], set()
    for h, w in sizes:
        d = E.one_plane(rs, h, w)
        if np.isnan(d).all() and not packer_only:
            d = rs.uniform(0.5, 10, (h, w)).astype(np.float32)
        if rs.rand() < 0.6 or long:
            planted |= plant_depth(rs, d, scale)
        depth.append(d)
    K = np.zeros((P, 3, 3))
    for p, (h, w) in enumerate(sizes):
        f = max(h, w)
        K[p] = [[(0.8 + 0.4 * rs.rand()) * f, 0.0, w / 2.0 + rs.uniform(-0.25, 0.25) * w], [0.0, (0.8 + 0.4 * rs.rand()) * f, h / 2.0 + rs.uniform(-0.25, 0.25) * h],
                [0.0, 0.0, 1.0]]
    # masks and logits: one stack per image
    mask_kind = ("u8", "bool")[rs.randint(2)]
    bytes_kind = int(rs.randint(3))
    logit_type = LOGIT_TYPES[rs.randint(3)]
    if fclass == "vec2":
        logit_type = {"f32": "f32", "f16": ("f16", "bf16")[rs.randint(2)], "u8": logit_type}[VEC2[sizes[0]]]
    threshold = THRESHOLDS[rs.randint(len(THRESHOLDS))]
    vals = np.array([1, 2, 0x80, 0xFF], np.uint8)
    stacks, mb, logits = [], [], []
    for p, (h, w) in enumerate(sizes):
        n = 0 if (p == none or long) else (int(rs.randint(1, 3)) if small_b else int(rs.randint(1, 5)))
        st = np.stack([E.one_mask(rs, h, w) for _ in range(n)]) if n else np.zeros((0, h, w), bool)
        if n and fclass in ("vec2", "gen2", "unpack"):
            st[0] = rs.rand(h, w) < 0.5                          # every word of the plane differs from its neighbours
        stacks.append(st)
        b = np.where(st, 1 if bytes_kind == 0 else (255 if bytes_kind == 1 else vals[rs.randint(0, 4, st.shape)]), 0).astype(np.uint8)
        mb.append(b.astype(bool) if mask_kind == "bool" else b)
        ls = np.stack([E.one_mask(rs, h, w) for _ in range(n)]) if n else np.zeros((0, h, w), bool)
        logits.append(logit_planes(rs, ls, threshold, logit_type))
    # label maps and the ids asked of them
    label_type = LABEL_TYPES[rs.randint(len(LABEL_TYPES))]
    okind = "u16" if label_type == "i16" else label_type
    maps, ids = [], []
    for p, (h, w) in enumerate(sizes):
        if long:
            maps.append(np.zeros((1, 1) + ((3,) if label_type == "rgb8" else ()), _encode_labels(np.zeros(1, np.int64), label_type).dtype)); ids.append([])
            continue
        pal = _palette(rs, label_type, 7)
        cells = blocky(rs, h, w, 6, max(2, h // 5), max(3, w // 6)) if rs.rand() < 0.7 else rs.randint(0, 6, (h, w))
        maps.append(_encode_labels(pal[cells], label_type))
        if p == none:
            ids.append([])
            continue
        row = [int(v) for v in pal[rs.permutation(6)[:int(rs.randint(1, 3 if small_b else 5))]]]
        if not small_b:
            if rs.rand() < 0.5:
                row.append(int(pal[6]) if int(pal[6]) not in pal[cells] else row[0])        # absent (pal[6] names no cell)
            if rs.rand() < 0.4:
                row.insert(int(rs.randint(len(row) + 1)), row[0])                          # repeated
            if OUTSIDE[okind] and rs.rand() < 0.5:
                row.append(int(OUTSIDE[okind][rs.randint(len(OUTSIDE[okind]))]))
        ids.append(row)
    B = {"masks": sum(len(s) for s in stacks), "logits": sum(len(s) for s in logits), "labels": sum(len(r) for r in ids)}
    img = {"masks": np.repeat(np.arange(P, dtype=np.int32), [len(s) for s in stacks]), "logits": np.repeat(np.arange(P, dtype=np.int32), [len(s) for s in logits]),
           "labels": np.repeat(np.arange(P, dtype=np.int32), [len(r) for r in ids])}
    broken = None
    if not packer_only and B["masks"] > 1 and rs.rand() < 0.125:
        broken = (BROKEN[rs.randint(len(BROKEN))], int(rs.randint(B["masks"])))
    lay = dict(base=int([1, 5, 16][rs.randint(3)]), extra=int([0, 3, 16, 40][rs.randint(4)]), canvas=(int(rs.randint(0, 4)), int([5, 16, 21, 32][rs.randint(4)])),
               reverse=bool(rs.randint(2)), perm={f: rs.permutation(B[f]) for f in ("masks", "logits")}, out_pad=int(rs.randint(1, 9)),
               pad_uniform=bool(rs.randint(2)), d16_pad=bool(rs.randint(2)) and not long, d16_extra=int([0, 5, 8][rs.randint(3)]))
    if fclass == "vec2":
        lay.update(base=16, extra=0)                             # (the aligned base and stride the vector form needs)
    return dict(seed=seed, P=P, sizes=sizes, uniform=uniform, fclass=fclass, w_in=w_in, packer_only=packer_only, none=none, depth=depth, K=K,
                scale=scale, planted=planted, mask_kind=mask_kind, bytes_kind=bytes_kind, logit_type=logit_type, threshold=threshold, stacks=stacks,
                mb=mb, logits=logits, label_type=label_type, maps=maps, ids=ids, B=B, img=img, broken=broken, lay=lay,
                fit_src=FAMILIES[rs.randint(3)], fit16=("f16", "u16h", "u16n")[rs.randint(3)])


def features(c):
    """What a case brings to a slice, from the generator alone -> set of names (tests/test_differential_checkers.py::
    test_format_slice_covers lists the ones a slice must hold)."""
    f = {f"class {c['fclass']}", f"masks {c['mask_kind']}", f"u8 bytes {c['bytes_kind']}", f"labels {c['label_type']}", f"logits {c['logit_type']}",
         f"threshold {c['threshold']!r}", "one size" if c["uniform"] else "mixed sizes", f"scale {c['scale']!r}"}
    f |= {f"frame {h}x{w}" for h, w in c["sizes"]} | {f"depth: {n}" for n in c["planted"]}
    if c["fclass"] == "unpack":
        f.add(f"unpack {c['w_in']}/{c['sizes'][0][1]}")
    if c["broken"]:
        f.add(f"broken: {c['broken'][0]}")
    for r in RUNS:
        if applies(c, r):
            f.add(f"run {run_name(r)}: {'one size' if c['uniform'] else 'mixed sizes'}")
    lay, (H, W) = c["lay"], c["sizes"][0]
    if c["uniform"] and c["fclass"] != "long":
        f.add(f"device base {lay['base']}")
        f.add("plane stride above H*W" if lay["extra"] else "plane stride H*W")
        f.add("u8 plane stride: multiple of 16 bytes" if (H * W + lay["extra"]) % 16 == 0 else "u8 plane stride: no multiple of 16 bytes")
        for elem in ("u8", c["logit_type"]):
            for pad in (False, True):
                W_out = padded_width(W) if pad else W
                if pack_trips(H, W, W_out, elem) > 1:
                    f.add(f"second trip: {'vector' if vec_form(H, W, W_out, elem) else 'general'} packer, {elem}")
                    if c["fclass"] == "vec2" and not pad and ELEM_BYTES[elem] == ELEM_BYTES[VEC2[(H, W)]]:
                        f.add(f"second trip at its smallest frame {H}x{W}: vector packer, {elem}")
        if unpack_trips(H, W) > 1 and W % 4 == 0:
            f.add("second trip: unpacker, quad form")
    if c["fclass"] == "long":
        tp, tu = depth_trips(1, *LONG, 1)
        f.add(f"depth trips {tp}/{tu}")
    if c["fclass"] != "long":
        f |= {"u8 canvas pitch: multiple of 16 bytes" if (w + lay["canvas"][1]) % 16 == 0 else "u8 canvas pitch: no multiple of 16 bytes" for _, w in c["sizes"]}
    if lay["reverse"] and c["P"] > 1:
        f.add("lowest data_ptr is not the first image's")
    if c["none"] is not None:
        f.add("an image with a (0, H, W) stack and no ids")
    ids = [i for row in c["ids"] for i in row]
    vals = [set(np.unique(label_values(m, c["label_type"])).tolist()) for m in c["maps"]]
    from tests.test_gpu_labels import OUTSIDE
    out = OUTSIDE["u16" if c["label_type"] == "i16" else c["label_type"]]
    if any(i in out for i in ids):
        f.add("ids outside the dtype's range")
    if any(i not in vals[p] and i not in out for p, row in enumerate(c["ids"]) for i in row):
        f.add("absent ids")
    if any(len(set(row)) < len(row) for row in c["ids"]):
        f.add("repeated ids")
    if any(i < 0 and i not in out for i in ids) or (c["label_type"] == "i16" and any(i >= 0x8000 for i in ids)):
        f.add("negative ids")
    if has_fit(c):
        f.add("fit leg")
        f.add(f"fit16 {c['fit16']}")
    return f


# ------------------------------------------------------------------------------------------------------------------------------
# oracle
# ------------------------------------------------------------------------------------------------------------------------------
def meant(c, fam):
    """The masks a family's rows mean, in image order -> list of bool (H_p, W_p)."""
    if fam == "masks":
        return [np.asarray(m) != 0 for st in c["mb"] for m in st]
    if fam == "logits":
        return [logit_mask(m, c["threshold"], c["logit_type"]) for st in c["logits"] for m in st]
    return [label_values(c["maps"][p], c["label_type"]) == i for p, row in enumerate(c["ids"]) for i in row]


def plane_words(mask, W_stored):
    """np.packbits, LSB first, of a mask on rows zero-padded to the stored width -> uint32 words (the last one zero-filled)."""
    h, w = mask.shape
    m = np.zeros((h, W_stored), bool)
    m[:, :w] = mask
    b = np.packbits(m.reshape(-1), bitorder="little")
    b = np.concatenate([b, np.zeros(-len(b) % 4, np.uint8)])
    return b.view(np.uint32)


def words_mask(words, H, W_stored, fw):
    """the inverse: uint32 words -> bool (H, fw)"""
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:H * W_stored]
    return bits.reshape(H, W_stored)[:, :fw].astype(bool)


def fit_oracle(c, masks, img, planes):
    """The reference fit of every row -> (records (B,39), status, n_valid, kappa, gap)."""
    from oracle import la3d_oracle as O

    B = len(masks)
    rec, st, nv, kap, gap = np.full((B, 39), np.nan), np.zeros(B, np.int32), np.zeros(B, np.int64), np.full(B, np.nan), np.full(B, np.nan)
    clouds = {}
    for n in range(B):
        p = int(img[n])
        if p not in clouds:
            clouds[p] = O.depth_to_points(planes[p][None], c["K"][p])
        rec[n], st[n], aux = O.fit_points(clouds[p][masks[n]], None, False, "pca")
        nv[n], kap[n], gap[n] = aux["n_valid"], aux.get("kappa", np.nan), aux.get("gap", np.nan)
    return rec, st, nv, kap, gap


def expected(c):
    """The oracle's result of a case -> dict: masks / area / stats per family, d16 (per dtype the stored words and both up-conversions of
    every image) and - cases with a fit leg - fit: per depth kind the reference records of the family the case fits."""
    from oracle import la3d_oracle as O

    want = dict(masks={}, area={}, stats={})
    for fam in FAMILIES:
        ms = meant(c, fam)
        want["masks"][fam] = ms
        want["area"][fam] = np.asarray([int(m.sum()) for m in ms], np.int64)
        want["stats"][fam] = {b: np.asarray([O.mask_stats(m, b) for m in ms], np.int64).reshape(len(ms), 4) for b in (10, 3)} if c["fclass"] != "long" else None
    d16 = {}
    for dt in ("f16", "u16"):
        stored = [quantise(d, dt, c["scale"]) for d in c["depth"]]
        d16[dt] = dict(words=stored, values={hole: [upconvert(s, c["scale"], hole) for s in stored] for hole in (True, False)})
    want["d16"] = d16
    if has_fit(c):
        fam = c["fit_src"]
        k16 = c["fit16"]
        planes16 = d16["f16" if k16 == "f16" else "u16"]["values"][k16 != "u16n"]
        want["fit"] = {"f32": fit_oracle(c, want["masks"][fam], c["img"][fam], c["depth"]), "16": fit_oracle(c, want["masks"][fam], c["img"][fam], planes16)}
    return want


_WANT = {}


def oracle_case(seed):
    """expected(make_case(seed)), kept for the process (the CPU tests and the GPU slice share it)."""
    if seed not in _WANT:
        _WANT[seed] = expected(make_case(seed))
    return _WANT[seed]


# ------------------------------------------------------------------------------------------------------------------------------
# GPU runs
# ------------------------------------------------------------------------------------------------------------------------------
RUNS = [dict(src=f, entry="frames", layout="host") for f in ("masks", "logits")] + [dict(src="labels", entry="frames", ids="host")] + \
       [dict(src=f, entry="frames", layout="device") for f in ("masks", "logits")] + [dict(src="labels", entry="frames", ids="device")] + \
       [dict(src=f, entry="uniform", layout="host", frame_pad=pad) for f in ("masks", "logits") for pad in (True, False)] + \
       [dict(src=f, entry="uniform", layout="device") for f in ("masks", "logits")] + \
       [dict(src="labels", entry="uniform", ids="host", frame_pad=True), dict(src="labels", entry="uniform", ids="device", frame_pad=False)] + \
       [dict(entry="unpack"), dict(entry="depth16", dtype="f16"), dict(entry="depth16", dtype="u16"),
        dict(entry="fit", form="uniform", depth="f32"), dict(entry="fit", form="uniform", depth="16"),
        dict(entry="fit", form="frames", depth="f32"), dict(entry="fit", form="frames", depth="16")]


def run_name(r):
    return " ".join(str(v) for v in r.values())


def has_fit(c):
    return not c["packer_only"] and not c["broken"] and c["B"][c["fit_src"]] > 0


def applies(c, r):
    """The depth packers take every case; the long frame takes nothing else; the uniform entries need images of one size; the
    hand-made MaskBits their case; the fit leg stays off the packer-only frames and the broken inputs."""
    e = r["entry"]
    if e == "depth16":
        return True
    if c["fclass"] == "long":
        return False
    if e == "unpack":
        return c["fclass"] == "unpack" and c["B"]["masks"] > 0
    if e == "fit":
        return has_fit(c) and (c["uniform"] or r["form"] == "frames")
    if c["B"][r["src"]] == 0 and e == "uniform":
        return False
    return c["uniform"] or e == "frames"


def family(r):
    return r.get("src")


def uniform_pad(c, r):
    """frame_pad of a uniform run (the device runs draw it per case; the second-trip frames pin the form they aim at)."""
    if "frame_pad" in r:
        return r["frame_pad"]
    if c["fclass"] in ("vec2", "gen2"):
        return c["sizes"][0] == GEN2[1]
    return c["lay"]["pad_uniform"]


def _torch_of(a, T, dev):
    """stored patterns / bytes / labels as the device tensor of their type"""
    import torch

    a = np.ascontiguousarray(a)
    if T == "bf16":
        return torch.as_tensor(a.view(np.int16), device=dev).view(torch.bfloat16)
    if T == "f16":
        return torch.as_tensor(a.view(np.float16), device=dev)
    if T == "f32":
        return torch.as_tensor(a.view(np.float32), device=dev)
    if a.dtype == np.uint16:
        return torch.as_tensor(a.view(np.int16), device=dev)
    return torch.as_tensor(a, device=dev)


def _host_of(a, T):
    """what a caller holds on the host (NumPy has no bfloat16: those go up as tensors)"""
    import torch

    if T == "bf16":
        return torch.as_tensor(np.ascontiguousarray(a).view(np.int16)).view(torch.bfloat16)
    return {"f16": lambda: a.view(np.float16), "f32": lambda: a.view(np.float32)}.get(T, lambda: a)()


def _strided(flat_t, B, H, W, base, stride):
    return flat_t.as_strided((B, H, W), (stride, W, 1), base)


def run_gpu(c, r, cache=None):
    """One run of a case on the GPU -> dict of NumPy arrays (see check_run).  `cache`: a dict kept across the runs of one case - the
    host runs leave the planes they wrote there and the fit leg fits those (it packs its own only when run alone).  Raises what the
    call raises."""
    import torch

    import labelany3d_amd as la
    from labelany3d_amd import frames as FR

    cache = {} if cache is None else cache
    dev = "cuda"
    np_ = lambda t: t.detach().cpu().numpy()   # noqa: E731
    u32 = lambda t: np_(t).view(np.uint32)     # noqa: E731
    e, fam, lay, P = r["entry"], r.get("src"), c["lay"], c["P"]
    T = c["logit_type"] if fam == "logits" else "u8"
    got = dict(sent=None)

    def tail(mb_):
        """unpacker and statistics of MaskBits a run returned"""
        out = dict(unpacked=np_(la.unpack_mask_bits(mb_)))
        if mb_.H * mb_.W <= 1 << 20:
            out["stats"] = {b: np_(la.mask_stats_bits(mb_, b)) for b in (10, 3)}
        return out

    def pack_frames_family(f, layout):
        """the FrameBits of a family's frames run (also what the fit leg fits) -> (FrameBits, order, buffer, total words)"""
        if f == "labels":
            pl = la.pack_label_frames(c["maps"], rgb=c["label_type"] == "rgb8")
            if layout == "device":
                flat = np.asarray([i for row in c["ids"] for i in row], np.int64)
                off = np.concatenate([[0], np.cumsum([len(row) for row in c["ids"]])])
                B = len(flat)
                stride = (pl.H * pl.W // 32 + 3) // 4 * 4
                buf = torch.full((max(B * stride, 4) + 8,), SENT, dtype=torch.int32, device=dev)
                fb = la.pack_label_bits_frames(pl, (torch.as_tensor(flat.astype(np.int32), device=dev), torch.as_tensor(off.astype(np.int32), device=dev)), out=buf)
            else:
                buf = None
                fb = la.pack_label_bits_frames(pl, c["ids"])
            return fb, np.arange(c["B"]["labels"]), buf
        src = c["mb"] if f == "masks" else c["logits"]
        Tt = "u8" if f == "masks" else c["logit_type"]
        if layout == "host":
            pm = la.pack_mask_frames([_host_of(s, Tt) for s in src])
            return la.pack_mask_bits_frames(pm, threshold=c["threshold"]), np.arange(c["B"][f]), None
        # device stacks read in place: every stack the top-left crop of a canvas in one allocation, the images in reverse order when
        # the case says so (the lowest data_ptr() is then the last image's); rows permuted; out= filled with SENT
        eh, ew = lay["canvas"]
        shapes = [(len(s), s.shape[1] + eh, s.shape[2] + ew) for s in src]
        sizes_el = [n * h * w for n, h, w in shapes]
        order_p = list(range(P))[::-1] if lay["reverse"] else list(range(P))
        starts, at = {}, lay["base"]
        for p in order_p:
            starts[p] = at
            at += sizes_el[p] + 3
        fill = (np.uint8(0xFF) if f == "masks" else pat_of(key_inf(Tt), Tt)[()])        # outside the crops: set / +inf
        host = np.full(at + 64, fill, src[0].dtype if src[0].dtype != np.bool_ else np.uint8)
        for p in range(P):
            n, h, w = shapes[p]
            if n:
                host[starts[p]:starts[p] + sizes_el[p]].reshape(n, h, w)[:, :h - eh, :w - ew] = src[p]
        flat_t = _torch_of(host, Tt, dev)
        if f == "masks" and c["mask_kind"] == "bool":
            flat_t = flat_t.view(torch.bool)
        stacks_t = []
        for p in range(P):
            n, h, w = shapes[p]
            stacks_t.append(flat_t.as_strided((n, h - eh, w - ew), (h * w, w, 1), starts[p]))
        pm = la.pack_mask_frames(stacks_t)
        B = c["B"][f]
        perm = lay["perm"][f]
        ii_h = c["img"][f][perm]
        offs_h, total = FR.frame_bits_offsets(pm.table_host, ii_h)
        t = torch.as_tensor(perm, device=dev)
        pitch = pm.pitch if pm.pitch is not None else torch.as_tensor(np.asarray([c["sizes"][p][1] for p in c["img"][f]], np.int32), device=dev)
        so, pi, ii, bo = pm.offsets[t].clone(), pitch[t].clone(), pm.image_index[t].clone(), torch.as_tensor(offs_h, device=dev)
        if c["broken"] and f == "masks":
            what, row = c["broken"]
            if what == BROKEN[0]:
                so[row] = -8
            elif what == BROKEN[1]:
                pi[row] = c["sizes"][int(ii_h[row])][1] - 1
            elif what == BROKEN[2]:
                ii[row] = P if row % 2 else -1
            elif what == BROKEN[3]:
                bo[row] = -4
            else:
                bo[row] = bo[row] + 2
        pm = pm._replace(offsets=so, pitch=pi, image_index=ii, bits_offsets=bo, bits_words=total)
        buf = torch.full((max(total, 4) + 8,), SENT, dtype=torch.int32, device=dev)
        return la.pack_mask_bits_frames(pm, threshold=c["threshold"], out=buf), perm, buf

    if e == "frames":
        fb, order, buf = pack_frames_family(fam, r.get("layout", r.get("ids")))
        torch.cuda.synchronize()
        got.update(buf=u32(fb.bits if buf is None else buf), offsets=np_(fb.offsets), image_index=np_(fb.image_index), area=np_(fb.area), H=fb.H, W=fb.W,
                   order=np.asarray(order), sent=None if buf is None else SENT)
        if buf is None:
            cache[("fb", fam)] = fb                             # the planes the fit leg fits
    elif e == "uniform":
        H, W = c["sizes"][0]
        pad = uniform_pad(c, r)
        W_out = padded_width(W) if pad else W
        nwords = (H * W_out + 31) // 32
        dev_layout = r.get("layout") == "device" or r.get("ids") == "device"
        B = c["B"][fam]
        out = torch.full((B, nwords + lay["out_pad"]), SENT, dtype=torch.int32, device=dev) if dev_layout else None
        if fam == "labels":
            rgb = c["label_type"] == "rgb8"
            maps = np.stack(c["maps"])
            ids = c["ids"]
            if dev_layout:
                ch = 3 if rgb else 1
                stride = (H * W + lay["extra"]) * ch
                base = lay["base"] * ch
                host = np.zeros(base + P * stride + 16, maps.dtype)
                for p in range(P):
                    host[base + p * stride:base + p * stride + H * W * ch] = maps[p].reshape(-1)
                flat_t = _torch_of(host, "labels", dev)
                if c["label_type"] == "u16":
                    flat_t = flat_t.view(torch.uint16)
                maps = flat_t.as_strided((P, H, W, 3), (stride, W * 3, 3, 1), base) if rgb else flat_t.as_strided((P, H, W), (stride, W, 1), base)
                flat = np.asarray([i for row in c["ids"] for i in row], np.int64)
                off = np.concatenate([[0], np.cumsum([len(row) for row in c["ids"]])])
                ids = (torch.as_tensor(flat.astype(np.int32), device=dev), torch.as_tensor(off.astype(np.int32), device=dev))
            lb = la.pack_label_bits(maps, ids, frame_pad=pad, rgb=rgb, out=out)
            bits = lb.bits
            got.update(area=np_(lb.area), image_index=np_(lb.image_index))
        else:
            src = np.concatenate(c["mb"] if fam == "masks" else c["logits"])
            if dev_layout:
                stride = H * W + lay["extra"]
                host = np.zeros(lay["base"] + B * stride + 16, src.dtype if src.dtype != np.bool_ else np.uint8)
                for n in range(B):
                    host[lay["base"] + n * stride:lay["base"] + n * stride + H * W] = src[n].reshape(-1)
                flat_t = _torch_of(host, T, dev)
                if fam == "masks" and c["mask_kind"] == "bool":
                    flat_t = flat_t.view(torch.bool)
                x = _strided(flat_t, B, H, W, lay["base"], stride)
            else:
                x = _host_of(src, T)
            bits = la.pack_mask_bits(x, frame_pad=pad, out=out) if fam == "masks" else la.pack_logits_bits(x, threshold=c["threshold"], frame_pad=pad, out=out)
        torch.cuda.synchronize()
        got.update(buf=u32(bits.bits), H=bits.H, W=bits.W, fw=bits.frame_width, sent=SENT if dev_layout else None, **tail(bits))
        if not dev_layout and pad:
            cache[("bits", fam)] = bits                         # the planes the fit leg fits
    elif e == "unpack":
        (H, fw), w_in = c["sizes"][0], c["w_in"]
        words = np.stack([plane_words(m, w_in) for m in meant(c, "masks")])
        mbits = la.MaskBits(torch.as_tensor(words.view(np.int32), device=dev), H, w_in, fw)
        got.update(buf=words, H=H, W=w_in, fw=fw, **tail(mbits))
    elif e == "depth16":
        dt = r["dtype"]
        words, values, bufs = [], {True: [], False: []}, []
        pad = lay["d16_pad"]
        groups = [list(range(P))] if c["uniform"] else [[p] for p in range(P)]
        for g in groups:
            H, W = c["sizes"][g[0]]
            W_out = padded_width(W) if pad else W
            stack = np.stack([c["depth"][p] for p in g])
            if c["uniform"] and c["fclass"] != "long":
                # device planes read in place, an out= whose planes lie further apart
                stride = H * W + lay["extra"]
                host = np.zeros(lay["base"] + len(g) * stride + 4, np.float32)
                for n in range(len(g)):
                    host[lay["base"] + n * stride:lay["base"] + n * stride + H * W] = stack[n].reshape(-1)
                x = _strided(torch.as_tensor(host, device=dev), len(g), H, W, lay["base"], stride)
                ostride = H * W_out + lay["d16_extra"]
                obuf = torch.full((len(g) * ostride + 8,), SENT16, dtype=torch.int16, device=dev)
                out = obuf.view(torch.float16 if dt == "f16" else torch.uint16).as_strided((len(g), H, W_out), (ostride, W_out, 1), 0)
                d = la.pack_depth16(x, dtype=dt, scale=c["scale"], frame_pad=pad, out=out)
                torch.cuda.synchronize()
                bufs.append((np_(obuf).view(np.uint16), ostride, H * W_out, len(g)))
            else:
                d = la.pack_depth16(stack if len(g) > 1 else stack[0], dtype=dt, scale=c["scale"], frame_pad=pad)
            data = d.data if d.data.dim() == 3 else d.data[None]
            w = np_(data.view(torch.int16)).view(np.uint16)
            words += [w[n] for n in range(len(g))]
            for hole in ((True, False) if dt == "u16" else (True,)):
                v = la.unpack_depth16(d._replace(zero_is_hole=hole))
                v = np_(v if v.dim() == 3 else v[None])
                values[hole] += [v[n] for n in range(len(g))]
        got.update(words=words, values=values, bufs=bufs, pad=pad)
    else:   # the fit leg: on the planes the packers just wrote
        f = c["fit_src"]
        img = c["img"][f]
        k16 = c["fit16"]
        dt = "f16" if k16 == "f16" else "u16"
        if r["form"] == "uniform":
            H, W = c["sizes"][0]
            bits = cache.get(("bits", f))
            if bits is not None:
                pass
            elif f == "labels":
                bits = la.pack_label_bits(np.stack(c["maps"]), c["ids"], rgb=c["label_type"] == "rgb8").bits
            elif f == "masks":
                bits = la.pack_mask_bits(np.concatenate(c["mb"]))
            else:
                bits = la.pack_logits_bits(_host_of(np.concatenate(c["logits"]), c["logit_type"]), threshold=c["threshold"])
            depth = np.stack(c["depth"])
            if r["depth"] == "16":
                depth = la.pack_depth16(depth, dtype=dt, scale=c["scale"], frame_pad=True)._replace(zero_is_hole=k16 != "u16n")
            b, st, aux = la.fit_instances_bits(depth, bits, c["K"], image_index=img)[:3]
        else:
            fb = cache.get(("fb", f))
            if fb is None:
                fb, _, _ = pack_frames_family(f, "host")
            if r["depth"] == "16":
                stored = [np_(la.pack_depth16(d, dtype=dt, scale=c["scale"]).data.view(torch.int16)).view(np.float16 if dt == "f16" else np.uint16) for d in c["depth"]]
                pf = la.pack_frames(stored, dtype=dt, scale=c["scale"], zero_is_hole=k16 != "u16n")
            else:
                pf = la.pack_frames(c["depth"])
            res = la.fit_instances_frames_bits(pf, fb, c["K"])
            b, st, aux = res["boxes"], res["status"], res["aux"]
        got.update(boxes=np_(b), status=np_(st), aux=np_(aux))
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# the checker
# ------------------------------------------------------------------------------------------------------------------------------
RULES = ("words", "padding", "area", "layout", "sentinel", "roundtrip", "stats", "depth16", "agree", "fit")


def decoded(c, r, got):
    """The planes of a pack run as bool masks in the case's row order (what `agree` compares) -> list, None for a row the run's
    layout does not let one read."""
    fam = family(r)
    B = c["B"][fam]
    if r["entry"] == "uniform":
        return [words_mask(got["buf"][n, :(got["H"] * got["W"] + 31) // 32], got["H"], got["W"], got["fw"]) for n in range(B)]
    out = [None] * B
    for i, n in enumerate(got["order"]):
        h, w = c["sizes"][int(c["img"][fam][n])]
        o, nw = int(got["offsets"][i]), h * padded_width(w) // 32
        if 0 <= o and o + nw <= len(got["buf"]):
            out[int(n)] = words_mask(got["buf"][o:o + nw], h, padded_width(w), w)
    return out


def check_run(c, want, r, got, default=None, rules=RULES, tally=None):
    """Compare one run's GPU output (run_gpu's dict) with want = expected(c).  `default`: decoded(...) of the family's first run of the
    case, for `agree`.  Returns the failures as strings (empty: the run agrees).  `rules`: the rules to apply."""
    e, fam = r["entry"], family(r)
    fails = []
    t = new_tally() if tally is None else tally
    tag = lambda n: f"row {n} (image {int(c['img'][fam][n])}, {c['sizes'][int(c['img'][fam][n])]})"   # noqa: E731
    if e in ("frames", "uniform", "unpack"):
        fam = fam or "masks"
        masks, B = want["masks"][fam], c["B"][fam]
        img = c["img"][fam]
    if e == "frames":
        order = got["order"]
        dev_ids = r.get("ids") == "device"
        Hb, Wb = max(h for h, _ in c["sizes"]), max(padded_width(w) for _, w in c["sizes"])
        if dev_ids:
            stride = (Hb * Wb // 32 + 3) // 4 * 4
            offs_w, total = np.arange(B, dtype=np.int64) * stride, B * stride
        else:
            offs_w, total = bits_offsets(c["sizes"], img[order])
        broke = c["broken"] if (c["broken"] and fam == "masks" and r.get("layout") == "device") else None
        offs_real = offs_w.copy()
        if "layout" in rules:
            if broke and broke[0] in BROKEN[3:]:
                offs_real[broke[1]] = -4 if broke[0] == BROKEN[3] else offs_w[broke[1]] + 2
            ii_w = img[order].copy()
            if broke and broke[0] == BROKEN[2]:
                ii_w[broke[1]] = c["P"] if broke[1] % 2 else -1
            if (got["H"], got["W"]) != (Hb, Wb):
                fails.append(f"layout: bounds {(got['H'], got['W'])}, expected {(Hb, Wb)}")
            if got["offsets"].shape != offs_real.shape or (got["offsets"] != offs_real).any():
                fails.append(f"layout: offsets {got['offsets'][:6].tolist()}, expected {offs_real[:6].tolist()}")
            if got["image_index"].shape != ii_w.shape or (got["image_index"] != ii_w).any():
                fails.append(f"layout: image_index {got['image_index'][:8].tolist()}, expected {ii_w[:8].tolist()}")
        buf = got["buf"]
        written = np.zeros(len(buf), bool)
        area_w = want["area"][fam][order].copy()
        for i, n in enumerate(order):
            h, w = c["sizes"][int(img[n])]
            nw, o = h * padded_width(w) // 32, int(offs_w[i])
            ww = plane_words(masks[n], padded_width(w))
            if broke and broke[1] == i:
                area_w[i] = 0
                if broke[0] in BROKEN[2:]:
                    continue                                     # untouched: the sentinel rule holds its words
                ww = np.zeros_like(ww)
            written[o:o + nw] = True
            g = buf[o:o + nw]
            t["planes"] += 1; t["words"] += nw
            if "words" in rules and (len(g) != nw or (g != ww).any()):
                bad = np.flatnonzero(g != ww) if len(g) == nw else []
                fails.append(f"words: {len(bad)} of {nw} differ in {tag(n)}: word {bad[:3].tolist()} got {[hex(v) for v in g[bad[:3]]]} expected {[hex(v) for v in ww[bad[:3]]]}")
            if "padding" in rules and len(g) == nw and w % 32:
                cols = np.unpackbits(np.ascontiguousarray(g).view(np.uint8), bitorder="little").reshape(h, padded_width(w))[:, w:]
                if cols.any():
                    fails.append(f"padding: {int(cols.sum())} bits set in the columns >= {w} of {tag(n)}")
        if "area" in rules and (got["area"].shape != area_w.shape or (got["area"] != area_w).any()):
            bad = np.flatnonzero(got["area"] != area_w) if got["area"].shape == area_w.shape else []
            fails.append(f"area: rows {bad[:4].tolist()} got {got['area'][bad[:4]].tolist() if len(bad) else got['area'].shape} expected {area_w[bad[:4]].tolist()}")
        if "sentinel" in rules and got["sent"] is not None:
            bad = np.flatnonzero(~written & (buf != np.uint32(got["sent"])))
            if len(bad):
                fails.append(f"sentinel: {len(bad)} words written outside the planes (first at word {int(bad[0])} of {len(buf)}, the planes end at {total})")
    elif e in ("uniform", "unpack"):
        H, fw = c["sizes"][0]
        W_st = c["w_in"] if e == "unpack" else (padded_width(fw) if uniform_pad(c, r) else fw)
        nw = (H * W_st + 31) // 32
        if "layout" in rules:
            if (got["H"], got["W"], got["fw"]) != (H, W_st, fw):
                fails.append(f"layout: (H, W, frame_width) = {(got['H'], got['W'], got['fw'])}, expected {(H, W_st, fw)}")
            if fam == "labels" and e == "uniform" and (got["image_index"].shape != img.shape or (got["image_index"] != img).any()):
                fails.append(f"layout: image_index {got['image_index'][:8].tolist()}, expected {img[:8].tolist()}")
        buf = got["buf"]
        if buf.shape[0] != B or buf.shape[1] < nw:
            return fails + [f"words: the planes are {buf.shape}, expected {(B, nw)}: nothing compared"]
        for n in range(B if e == "uniform" else 0):
            ww, g = plane_words(masks[n], W_st), buf[n, :nw]
            t["planes"] += 1; t["words"] += nw
            if "words" in rules and (g != ww).any():
                bad = np.flatnonzero(g != ww)
                fails.append(f"words: {len(bad)} of {nw} differ in {tag(n)}: word {bad[:3].tolist()} got {[hex(v) for v in g[bad[:3]]]} expected {[hex(v) for v in ww[bad[:3]]]}")
            if "padding" in rules:
                bits = np.unpackbits(np.ascontiguousarray(g).view(np.uint8), bitorder="little")
                if bits[H * W_st:].any() or bits[:H * W_st].reshape(H, W_st)[:, fw:].any():
                    fails.append(f"padding: bits set in the columns >= {fw} or behind pixel {H * W_st} of {tag(n)}")
        if "area" in rules and e == "uniform" and fam == "labels" and (got["area"] != want["area"][fam]).any():
            bad = np.flatnonzero(got["area"] != want["area"][fam])
            fails.append(f"area: rows {bad[:4].tolist()} got {got['area'][bad[:4]].tolist()} expected {want['area'][fam][bad[:4]].tolist()}")
        if "sentinel" in rules and got["sent"] is not None and (buf[:, nw:] != np.uint32(got["sent"])).any():
            fails.append(f"sentinel: words written behind the {nw} words of a plane (rows {np.flatnonzero((buf[:, nw:] != np.uint32(got['sent'])).any(1))[:4].tolist()})")
        if "roundtrip" in rules:
            want_m = np.stack(masks) if B else np.zeros((0, H, fw), bool)
            if got["unpacked"].shape != want_m.shape or got["unpacked"].dtype != np.bool_:
                fails.append(f"roundtrip: unpack_mask_bits gave {got['unpacked'].shape} {got['unpacked'].dtype}, expected {want_m.shape} bool")
            elif (got["unpacked"] != want_m).any():
                bad = np.argwhere(got["unpacked"] != want_m)
                fails.append(f"roundtrip: {len(bad)} pixels differ, first (row, v, u) = {bad[0].tolist()} of {tag(int(bad[0][0]))} stored {W_st} wide")
        if "stats" in rules and "stats" in got:
            for b in (10, 3):
                if (got["stats"][b] != want["stats"][fam][b]).any():
                    bad = np.flatnonzero((got["stats"][b] != want["stats"][fam][b]).any(1))
                    fails.append(f"stats: boundary {b}: rows {bad[:4].tolist()} got {got['stats'][b][bad[0]].tolist()} expected {want['stats'][fam][b][bad[0]].tolist()}")
    elif e == "depth16":
        if "depth16" in rules:
            dt, w16 = r["dtype"], want["d16"][r["dtype"]]
            for p, (h, w) in enumerate(c["sizes"]):
                g = got["words"][p]
                t["depth_words"] += g.size
                if g.shape != (h, padded_width(w) if got["pad"] else w):
                    fails.append(f"depth16 {dt}: image {p} packed to {g.shape}")
                    continue
                if (g[:, :w] != w16["words"][p].view(np.uint16)).any():
                    bad = np.argwhere(g[:, :w] != w16["words"][p].view(np.uint16))
                    v, u = bad[0]
                    fails.append(f"depth16 {dt}: {len(bad)} words differ in image {p} {(h, w)}: pixel {(int(v), int(u))} depth {c['depth'][p][v, u]!r} scale {c['scale']!r} "
                                 f"got {int(g[v, u])} expected {int(w16['words'][p].view(np.uint16)[v, u])}")
                if g[:, w:].any():
                    fails.append(f"depth16 {dt}: padded columns of image {p} are not zero")
                for hole, vals in got["values"].items():
                    if not vals:
                        continue
                    a, b = vals[p], w16["values"][hole][p]
                    if a.shape != b.shape or a.dtype != np.float32 or not (((a != a) & (b != b)) | (a.view(np.uint32) == b.view(np.uint32))).all():
                        fails.append(f"depth16 {dt}: unpacked floats of image {p} differ (zero_is_hole={hole})")
            for obuf, ostride, n_el, P_ in got["bufs"]:
                live = np.zeros(len(obuf), bool)
                for n in range(P_):
                    live[n * ostride:n * ostride + n_el] = True
                if (obuf[~live] != SENT16).any():
                    fails.append(f"depth16 {dt}: {int((obuf[~live] != SENT16).sum())} words written between or behind the planes of out=")
    elif e == "fit" and "fit" in rules:
        fails += _check_fit(c, want, r, got, t)
    if "agree" in rules and default is not None and e in ("frames", "uniform"):
        mine = decoded(c, r, got)
        broke_row = None
        if c["broken"] and fam == "masks" and r.get("layout") == "device" and e == "frames":
            broke_row = int(got["order"][c["broken"][1]])
        bad = [n for n in range(len(mine)) if n != broke_row and (mine[n] is None or default[n] is None or mine[n].shape != default[n].shape or (mine[n] != default[n]).any())]
        if bad:
            fails.append(f"agree: the planes of rows {bad[:4]} differ from the first run of the family")
    return fails


def _check_fit(c, want, r, got, t):
    from tests.test_gpu_parity import assert_records, reference_axis_noise

    rec, st, nv, kap, gap_o = want["fit"][r["depth"]]
    fam = c["fit_src"]
    b, stg, aux = got["boxes"], got["status"], got["aux"]
    B = len(st)
    t["fitted"] += B
    if stg.shape != st.shape or (stg != st).any():
        bad = np.flatnonzero(stg != st) if stg.shape == st.shape else []
        return [f"fit: status at rows {bad[:5].tolist()}: got {stg[bad][:5].tolist() if len(bad) else stg.shape} expected {st[bad][:5].tolist()}"]
    ok = st == 0
    if not np.isnan(b[~ok]).all():
        return ["fit: a rejected instance's record is not NaN"]
    if not np.array_equal(aux[:, 2], want["area"][fam]):
        return [f"fit: n_masked differs at rows {np.flatnonzero(aux[:, 2] != want['area'][fam])[:4].tolist()}"]
    if not np.array_equal(aux[ok, 1], nv[ok]):
        return [f"fit: n_valid differs at rows {np.flatnonzero(ok)[aux[ok, 1] != nv[ok]][:4].tolist()}"]
    tie = ok & ~(aux[:, 3] >= 1e-9)
    # the don't-care class is the oracle's too: a reported gap below 1e-9 (or NaN) on a cloud whose own gap (np.longdouble moments,
    # O.pca_conditioning) is 1e-6 or more is a wrong gap, not a tie - it would take the record out of the comparison
    with np.errstate(invalid="ignore"):
        wrong = tie & (gap_o >= 1e-6)
    if wrong.any():
        bad = np.flatnonzero(wrong)
        return [f"fit: reported eigen-gap {aux[bad[0], 3]!r} at rows {bad[:4].tolist()}, where the oracle's gap is {gap_o[bad[0]]:.3g}: not a tie"]
    t["tied"] += int(tie.sum())
    noise = reference_axis_noise(kap, aux[:, 1], aux[:, 3])
    fails = []
    for n in np.flatnonzero(ok & ~tie):
        try:
            assert_records(b[n:n + 1], rec[n:n + 1], f"seed {c['seed']} {r}", gap=aux[n:n + 1, 3], noise=noise[n:n + 1])
            t["compared"] += 1
        except AssertionError as e:
            what = [ln for ln in str(e).splitlines() if "center" in ln or "R_cam" in ln or "vertices" in ln]
            fails.append(f"fit: record {n} (image {int(c['img'][fam][n])}): {what[0].strip() if what else 'mismatch'}; n_valid {int(aux[n, 1])} gap {aux[n, 3]:.3g} "
                         f"| d center/dims {np.abs(b[n, :6] - rec[n, :6]).max():.3g}")
    return fails


def new_tally():
    return dict(cases=0, rows=0, pixels=0, calls={}, planes=0, words=0, depth_words=0, fitted=0, compared=0, tied=0)


def tally_case(t, c, want):
    t["cases"] += 1
    t["rows"] += sum(c["B"].values())
    t["pixels"] += int(sum(int(a.sum()) for a in want["area"].values()))


def tally_call(t, r):
    t["calls"][run_name(r)] = t["calls"].get(run_name(r), 0) + 1


def tally_lines(t):
    return [f"{t['cases']} cases ({t['rows']} mask, logit and label rows meaning {t['pixels']} pixels), {sum(t['calls'].values())} calls; {t['planes']} planes and {t['words']} words compared; {t['depth_words']} 16-bit depth words; "
            f"instances fitted / compared record by record / tied: {t['fitted']} / {t['compared']} / {t['tied']}"] + \
           [f"  calls of run {k}: {v}" for k, v in t["calls"].items()]
