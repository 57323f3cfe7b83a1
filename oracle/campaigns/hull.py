"""The randomised differential campaign over the convex-hull yaw of the depth + mask fit (la3d_fit_args::method =
LA3D_METHOD_CONVEX_HULL): case generator, coverage rule, oracle, GPU runs and the checker.  profiles/hull/fuzz_hull.py drives it at
scale; tests/test_gpu_differential.py runs a committed slice of its seeds (tests/campaign_slices.py::HULL_SEEDS).

One CASE = one hull call with the adversarial inputs of oracle/campaigns/engines.py (its masks, polygons and depth planes) on the
smallest frames at which the hull path can still go wrong, plus inputs aimed at the documented limits of full-mask mode
(include/la3d.h "convex-hull yaw"):
  frames on the tiled path   96x224, 128x160, 200x160, 240x320 (28 / 40 / 85 / 220 tiles of 32 x 8 pixels leave room for the column
                             arrays), 100x214 and 120x250 (padded to 224 / 256 columns by the wrappers), 480x640 (B <= 3)
  64x256                     the column arrays alone fill the bit image: every instance with a masked pixel is refused
  96x1056                    wider than the 1024 columns whose two ends the finish kernel always holds: bands of one row, of two rows
                             and of two rows of equal depth, with candidate counts either side of 2048
  off the tiled path         64x96 (24 tiles), 37x53 and tiny frames: refused as a whole in full-mask mode, fitted in subsample mode
  tile rectangles            masks whose active-tile count is the frame's room - 1, the room, the room + 1
  constant planes            with zero and negative depths sprinkled in: footprints with exactly parallel edges
About half of the cases run in full-mask mode, the rest in reference-subsample mode (sample_idx drawn as engines.make_case draws it).

covered(c, n, r) restates the documented coverage rule of full-mask mode in plain Python; check_run holds every run to it and to the
oracle: status exactly, a refused instance NaN throughout, n_masked / n_valid exactly - with the one exception include/la3d.h states:
an instance refused by the frame, the ground row, the skew or the active tiles leaves before its mask is counted and must report
n_valid 0 and n_masked NaN, while one refused for its candidate count reports both exactly - and every fitted record by its CLASS,
which is decided from the oracle alone (O.hull_edge_table):
  decided    the runner-up edge's rectangle is more than 1e-9 (relative) larger than the minimum: assert_records at its own tolerance
             and aux[3] <= -3, no waiver
  tied       another edge lies within 1e-9 of the minimum (parallel / perpendicular twins: the reference's pick among them is a coin
             toss of its own rounding): the GPU's yaw must be the yaw of one of those edges and its record the oracle's box UNDER
             that yaw (estimate_bbox(yaw=...)) - matching the area alone is not enough
  flat       the footprint of the oracle's box is at most 1e-9 extent^2 (the GPU's then has to be too), or the oracle fell back to PCA
             (fewer than 3 hull vertices): height and centre y to 1e-9; where both sides fell back, the PCA rule of engines.check_run

The oracle is test infrastructure: it is the checker here."""
import numpy as np

from . import engines as E

TILED = [(96, 224), (128, 160), (200, 160), (240, 320), (100, 214), (120, 250)]
BIG, ZERO_ROOM, WIDE, SMALL_OFF, ODD_OFF = (480, 640), (64, 256), (96, 1056), (64, 96), (37, 53)
BS = [1, 2, 3, 5, 8, 17, 33]
HCAP = 2048            # candidates the finish kernel holds (la3d.h)
SHARED_BYTES = 752     # the fit kernel's fixed LDS behind the bit image (la3d.h, rule 2; la3d_device.hpp holds struct Shared to it)
REL_TIE = 1e-9         # the project's tolerance for "the same area" (tests/test_gpu_hull_instances.py, oracle/campaigns/points.py)


# ------------------------------------------------------------------------------------------------------------------------------
# the documented coverage rule of full-mask mode
# ------------------------------------------------------------------------------------------------------------------------------
def padded_width(W):
    return (W + 31) // 32 * 32


def stored_width(W, r):
    """The row length the call runs on: every entry pads an odd width to the next multiple of 32 except la3d_fit_instances_ex with u8
    planes, which takes them as they lie."""
    return W if r.get("entry") == "ex_u8" else padded_width(W)


def bit_image_bytes(H, W):
    """la3d_device.hpp::mask_bit_bytes: H W / 8, whole 32-bit words, 16-byte granules."""
    return ((((H * W + 15) // 16 + 1) // 2) * 4 + 15) & ~15


def list_capacity(H, W):
    """Entries of the active-tile list (la3d_device.hpp::tiled_list_cap, full-mask mode): what the largest number of workgroups per
    CU (160 KiB of LDS, four at most) leaves behind bit image + Shared, once that is 256 entries or every tile of the frame."""
    ntiles = (W // 32) * ((H + 7) // 8)
    fixed = bit_image_bytes(H, W) + SHARED_BYTES
    cap, want = 0, min(ntiles, 256)
    for wg in (4, 3, 2, 1):
        if cap >= want:
            break
        cap = (((160 * 1024 // wg) & ~15) - fixed) // 2
    return min(cap, ntiles)


def on_tiled_path(H, W):
    """W: the stored width.  Word-aligned rows, 16-byte groups, at most 255 x 255 tiles, the bit image in LDS, a list of >= 64 tiles."""
    if W % 32 or (H * W) % 16 or W // 32 > 255 or (H + 7) // 8 > 255 or bit_image_bytes(H, W) > 128 * 1024:
        return False
    return list_capacity(H, W) >= 64


def column_room(H, W):
    """Active tiles that leave room for the column arrays: tiles x 32 B + 8 W bytes within the bit image."""
    return (bit_image_bytes(H, W) - 8 * W) // 32


def tile_room(H, W):
    """The largest active-tile count of a fitted instance on a frame of the tiled path: the column arrays fit behind the compacted
    tiles (column_room), the tiles and their depth-range words fit (tiles x 32 B + two words per tile in 16-byte granules + 384 B
    within the bit image), and the list holds them (list_capacity)."""
    n = min(column_room(H, W), list_capacity(H, W))
    while n > 0 and n * 32 + (((2 * n + 3) & ~3) + 96) * 4 > bit_image_bytes(H, W):
        n -= 1
    return max(n, 0)


def active_tiles(mask):
    H, W = mask.shape
    Wp, Hp = padded_width(W), (H + 7) // 8 * 8
    m = np.zeros((Hp, Wp), bool)
    m[:H, :W] = mask
    return int(m.reshape(Hp // 8, 8, Wp // 32, 32).any(axis=(1, 3)).sum())


def candidate_count(mask, depth):
    """Points the finish kernel builds its hull from: per pixel column the nearest and the farthest finite depth under the mask, ONE
    point where the two are the same float (-0 and +0 are two)."""
    d = np.ascontiguousarray(depth, np.float32)
    valid = mask & np.isfinite(d)
    b = d.view(np.uint32).astype(np.int64)
    key = np.where(b >> 31, b ^ 0xffffffff, b | 0x80000000)      # orders like the float, negative values included
    lo = np.where(valid, key, 1 << 40).min(axis=0)
    hi = np.where(valid, key, -1).max(axis=0)
    occ = hi >= 0
    return int(occ.sum() + (occ & (lo != hi)).sum())


def plane_of(c, n):
    return 0 if c["P"] == 1 else (int(c["image_index"][n]) if c["image_index"] is not None else n)


def covered(c, n, r=None):
    """Full-mask mode: is instance n of case c fitted by run r (None: the default u8 run)?  -> (True, None) or (False, reason), reason
    in REASONS, in the order the call decides: the frame (the whole call), then per instance ground row, skewed K, active tiles -
    each of which comes BEFORE the reference's own rejections (an empty mask, a degenerate ground row: status 5, not 1 / 2) - and
    last, for a cloud that has valid points, the candidate count."""
    r = {} if r is None else r
    H, W = c["H"], stored_width(c["W"], r)
    if not on_tiled_path(H, W):
        return False, "frame"
    if c["ground"] is not None and not np.isnan(c["ground"][n, 0]):
        return False, "ground"
    p = plane_of(c, n)
    if c["K"][p, 0, 1] != 0.0:
        return False, "skew"
    if active_tiles(c["masks"][n]) > tile_room(H, W):
        return False, "tiles"
    if candidate_count(c["masks"][n], c["depth"][p]) > HCAP:
        return False, "candidates"
    return True, None


REASONS = ("frame", "ground", "skew", "tiles", "candidates")


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
def tile_rect_mask(rs, H, W, ntarget):
    """A mask with exactly ntarget active tiles (32 x 8 pixels, rows of the padded frame): whole tile rows from a random first row, a
    partial row behind them, the tiles of the partial row and of the right edge touched in a few pixels only."""
    ntx, nty = padded_width(W) // 32, (H + 7) // 8
    ntarget = min(ntarget, ntx * nty)
    full, rem = divmod(ntarget, ntx)
    ty0 = rs.randint(0, nty - full - (1 if rem else 0) + 1)
    m = np.zeros((H, W), bool)
    m[ty0 * 8:(ty0 + full) * 8, :] = True
    if rs.rand() < 0.5 and full:                       # the last column of tiles holds one pixel column only
        m[ty0 * 8:(ty0 + full) * 8, (ntx - 1) * 32 + 1:] = False
    for tx in range(rem):
        r0, c0 = (ty0 + full) * 8, tx * 32
        rr, cc = r0 + rs.randint(0, min(8, H - r0)), c0 + rs.randint(0, min(32, W - c0))
        m[rr:min(rr + rs.randint(1, 9), r0 + 8, H), cc:min(cc + rs.randint(1, 33), c0 + 32, W)] = True
    assert active_tiles(m) == ntarget, (active_tiles(m), ntarget)
    return m


def band_case(rs, H, W, kind, count):
    """A band on the wide frame and the depth rows under it -> (mask, row0, rows of depth (1 or 2, W)): kind 0 one row, 1 two rows,
    2 two rows of equal depth within each column; `count` = the candidates it gives (kind 1: 2 x columns - the columns made equal)."""
    r0 = rs.randint(0, H - 1)
    base = (2.0 + rs.uniform(0, 3) + rs.uniform(-1, 1) * np.arange(W) / W + 0.05 * rs.randn(W)).astype(np.float32)
    m = np.zeros((H, W), bool)
    if kind == 0:
        ncol = min(count, W)
        c0 = rs.randint(0, W - ncol + 1)
        m[r0, c0:c0 + ncol] = True
        return m, r0, base[None]
    far = (base + rs.uniform(0.25, 1.0, W)).astype(np.float32)
    if kind == 2:
        ncol = min(count, W)
        c0 = rs.randint(0, W - ncol + 1)
        m[r0:r0 + 2, c0:c0 + ncol] = True
        return m, r0, np.stack([base, base])
    ncol = min((count + 1) // 2, W)
    equal = 2 * ncol - count                           # 0 or 1 columns whose two depths coincide
    c0 = rs.randint(0, W - ncol + 1)
    m[r0:r0 + 2, c0:c0 + ncol] = True
    for u in rs.choice(np.arange(c0, c0 + ncol), equal, replace=False):
        far[u] = base[u]
    return m, r0, np.stack([base, far])


def signed_constant_plane(rs, H, W):
    """A constant plane with zero and negative pixels sprinkled in: footprints of exactly parallel edges, points behind the camera."""
    v = np.float32(rs.uniform(0.3, 50))
    d = np.full((H, W), v, np.float32)
    bad = rs.rand(H, W) < 10 ** rs.uniform(-3, -1)
    vals = np.array([0.0, -0.0, -1.0, -v, -0.5 * v], np.float32)
    d[bad] = vals[rs.randint(0, len(vals), int(bad.sum()))]
    return d


def draw_frame(rs, full, poly):
    """(H, W, class) of a case."""
    u = rs.rand()
    if poly:                                           # (the oracle's rasteriser is a Python loop: the small frames)
        if not full and u < 0.25:
            return ODD_OFF + ("off",)
        return TILED[rs.randint(len(TILED))] + ("tiled",)
    if u < 0.55:
        return TILED[rs.randint(len(TILED))] + ("tiled",)
    if u < 0.62:
        return ZERO_ROOM + ("zero_room",)
    if u < 0.78:
        return WIDE + ("wide",)
    if u < 0.84:
        return BIG + ("big",)
    v = rs.rand()
    if v < 0.4:
        return (E.TINY_HS[rs.randint(len(E.TINY_HS))], E.TINY_WS[rs.randint(len(E.TINY_WS))], "off")
    return (ODD_OFF if v < 0.7 else SMALL_OFF) + ("off",)


def make_case(seed):
    """One case of the campaign (inputs only); the keys of engines.make_case plus full (full-mask mode), fclass (frame class) and
    aimed (per instance: None, or the boundary the mask was built for)."""
    rs = np.random.RandomState(seed)
    full = rs.rand() < 0.5
    poly_case = rs.rand() < 0.25
    H, W, fclass = draw_frame(rs, full, poly_case)
    B = BS[rs.randint(len(BS))]
    if fclass == "tiled" and (H, W) == (96, 224) and not poly_case and rs.rand() < 0.12:
        B = int(rs.choice([161, 300]))                 # across the batch limits of the other engines (160) and of the launch order (256)
    if fclass == "big":
        B = min(B, 3)
    if fclass == "wide":
        B = min(B, 8)
    if poly_case:
        B = min(B, 17)
    mode = rs.randint(0, 3)                            # 0: one shared plane, 1: private planes, 2: P planes + image_index
    if fclass == "wide" and full:
        mode = 1                                       # (the bands bring their own depth rows)
    P = 1 if mode == 0 else (B if mode == 1 else rs.randint(1, B + 1))
    signed = fclass in ("tiled", "big") and rs.rand() < 0.2
    depth, dkind = [], []
    for _ in range(P):
        if signed:
            depth.append(signed_constant_plane(rs, H, W)); dkind.append(5)
        else:
            depth.append(E.one_plane(rs, H, W)); dkind.append(E.one_plane.kind)
    depth = np.stack(depth)
    image_index = rs.randint(0, P, B).astype(np.int32) if mode == 2 and P > 1 else None
    if mode == 2 and P == 1:
        image_index = None
    skew = rs.rand() < 0.2
    K = np.zeros((P, 3, 3))
    for p in range(P):
        f = rs.uniform(0.4, 3.0) * W
        sk = rs.uniform(-5, 5) if skew and (P == 1 or rs.rand() < 0.5) else 0.0        # (several planes: some cameras skewed)
        K[p] = [[f, sk, W / 2 + rs.uniform(-0.3, 0.3) * W], [0, f * rs.uniform(0.8, 1.25), H / 2 + rs.uniform(-0.3, 0.3) * H], [0, 0, 1]]
    if rs.rand() < 0.5:
        K[:] = K[0]
    room = tile_room(H, padded_width(W)) if on_tiled_path(H, padded_width(W)) else 0
    masks, mkind, segs, aimed = [], [], [], []
    for n in range(B):
        p = 0 if P == 1 else (int(image_index[n]) if image_index is not None else n)
        u = rs.rand()
        if poly_case:
            m, seg = E.one_polygon_mask(rs, H, W)
            masks.append(m); mkind.append(14); segs.append(seg); aimed.append(None)
        elif fclass == "wide" and full and u < 0.8:
            kind = rs.randint(0, 3)
            count = int(rs.choice([2047, 2048, 2049, 2050, rs.randint(3, 2113)])) if kind == 1 else int(rs.choice([W, rs.randint(1, W + 1)]))
            m, r0, rows = band_case(rs, H, W, kind, count)
            depth[p, r0:r0 + len(rows)] = rows
            masks.append(m); mkind.append(15 + kind); aimed.append("candidates")
        elif fclass in ("tiled", "big") and full and room > 1 and u < 0.3:
            masks.append(tile_rect_mask(rs, H, W, room + rs.randint(-1, 2))); mkind.append(18); aimed.append("tiles")
        else:
            masks.append(E.one_mask(rs, H, W)); mkind.append(E.one_mask.kind); aimed.append(None)
    masks = np.stack(masks)
    mb = masks.astype(np.uint8)
    bytes_kind = rs.randint(0, 3)
    if bytes_kind == 1:
        mb *= 255
    elif bytes_kind == 2:
        mb = np.where(masks, rs.randint(1, 256, masks.shape), 0).astype(np.uint8)
    gu = rs.rand()
    gk = 0 if gu < (0.6 if full else 0.3) else (1 if gu < (0.95 if full else 0.65) else 2)   # none / some (NaN rows) / all
    ground = None
    if gk:
        ground = np.array([[0.05, -0.97, 0.1, 1.2]] * B) + 0.05 * rs.randn(B, 4)
        for n in range(B):
            u = rs.rand()
            if gk == 1 and u < (0.7 if full else 0.3):
                ground[n, 0] = np.nan                  # "no ground" for this instance
            elif u < 0.82:
                pass
            elif u < 0.92:
                ground[n] = [0, -1, 0, 1.0]            # already aligned: the reference's degenerate case (status 2)
            else:
                ground[n, :3] = 0.0
    sidx = None
    if not full:
        counts = masks.reshape(B, -1).sum(1)
        sidx = np.zeros((B, 500), np.int32)
        for n, cnt in enumerate(counts):
            if cnt > 500:
                sidx[n] = rs.randint(0, int(cnt), 500)
    return dict(seed=seed, H=H, W=W, B=B, P=P, depth=depth, K=K, masks=masks, mb=mb, ground=ground, image_index=image_index, sidx=sidx,
                skew=skew, mkind=mkind, dkind=dkind, segs=segs if poly_case else None, full=full, fclass=fclass, aimed=aimed)


# ------------------------------------------------------------------------------------------------------------------------------
# oracle
# ------------------------------------------------------------------------------------------------------------------------------
def classify(rec, table):
    """The class of a fitted record, from the oracle alone -> ("decided" | "tied" | "flat" | "fallback", indices of the edges within
    REL_TIE of the minimum)."""
    if table is None:
        return "fallback", np.zeros(0, int)
    yaws, areas = table
    amin = areas.min()
    ext = max(np.abs(rec[3:6]).max(), 1e-300)
    # flat: the footprint of the reference's own box (dz x dx) has no area - points collinear but for rounding, e.g. the one ray of a
    # single pixel column; whether such a cloud has a 2-D hull at all is decided by last bits.  (The table's `areas` are what the
    # reference minimises, :204-216 - the extent product under a turn by +yaw - not the area of the box it then writes.)
    if rec[3] * rec[5] <= 1e-9 * ext * ext:
        return "flat", np.zeros(0, int)
    near = np.flatnonzero(areas - amin <= REL_TIE * amin)
    return ("tied" if len(near) > 1 else "decided"), near


class Ref:
    """The oracle's result of one case: per instance status, record, n_valid, kappa, the hull edge table and the class - for the
    instances some run fits (full-mask mode: the covered ones) - and box_under(n, yaw)."""

    def __init__(self, c):
        from oracle import la3d_oracle as O

        self.c = c
        B = c["B"]
        self.rec = np.full((B, 39), np.nan)
        self.st = np.full(B, -1, np.int32)
        self.nv = np.zeros(B, np.int64)
        self.kap = np.full(B, np.nan)
        self.table = [None] * B
        self.cls = [None] * B
        self.near = [None] * B
        self.yaw = np.full(B, np.nan)
        self._pts = {}
        order = np.argsort([plane_of(c, n) for n in range(B)], kind="stable")   # (one plane's points at a time)
        cur, cloud = None, None
        for n in order:
            why = covered(c, n)[1] if c["full"] else None
            if why is not None and why != "candidates":
                continue                               # (refused by every run before the mask is counted: the oracle is never looked at)
            p = plane_of(c, n)
            if p != cur:
                cur, cloud = p, O.depth_to_points(c["depth"][p][None], c["K"][p])
            pts = cloud[c["masks"][n]]
            if why == "candidates":                    # refused behind the fit stage: n_valid is reported, the record never looked at
                self.nv[n] = O.fit_points(pts, None, False, "convex_hull")[2]["n_valid"]
                continue
            g = None if c["ground"] is None or np.isnan(c["ground"][n, 0]) else c["ground"][n]
            ri = np.asarray(c["sidx"][n]) if c["sidx"] is not None and len(pts) > O.SUBSAMPLE else False
            if ri is not False:
                pts, ri = pts[ri], False
            self._pts[n] = (pts, g)
            self.rec[n], self.st[n], aux = O.fit_points(pts, g, False, "convex_hull")
            self.nv[n], self.kap[n], self.yaw[n] = aux["n_valid"], aux.get("kappa", np.nan), aux["yaw"]
            if self.st[n] == 0:
                with np.errstate(invalid="ignore", over="ignore"):
                    rot = np.dot(pts, O.ground_rotation(g))
                rot = rot[~np.isnan(rot).any(axis=1)]
                self.table[n] = O.hull_edge_table(rot)
                self.cls[n], self.near[n] = classify(self.rec[n], self.table[n])

    def box_under(self, n, yaw):
        from oracle import la3d_oracle as O

        pts, g = self._pts[n]
        return O.fit_points(pts, g, False, "convex_hull", yaw=yaw)[0]


_REFS = {}


def oracle_case(seed):
    """Ref of make_case(seed), kept for the process (the CPU tests and the GPU slice share it)."""
    if seed not in _REFS:
        _REFS[seed] = Ref(make_case(seed))
    return _REFS[seed]


# ------------------------------------------------------------------------------------------------------------------------------
# GPU runs
# ------------------------------------------------------------------------------------------------------------------------------
# sources: u8 planes, run lengths, polygons (polygon cases), bit planes, la3d_fit_instances_ex with the 2-D boxes of the epilogue and an
# area hint (u8) and with the fused filter on top (run lengths); pins: documented as ignored by hull calls - the same bytes as the
# default run
SOURCES = [dict(), dict(entry="rle"), dict(entry="poly"), dict(entry="bits"), dict(entry="ex_u8"), dict(entry="ex_rle")]
PINS = [dict(engine="rows"), dict(engine="band"), dict(engine="split"), dict(build="plain")]
RUNS = SOURCES + PINS
EX_ENTRIES = ("ex_u8", "ex_rle")


def applies(c, r):
    """Polygon runs need a polygon case; a full-mask case on a frame off the tiled path is refused as a whole: once, not per run."""
    if r.get("entry") == "poly" and c["segs"] is None:
        return False
    if c["full"] and r and not on_tiled_path(c["H"], padded_width(c["W"])):
        return False
    return True


def run_gpu(c, r, cache=None):
    """One run of a case on the GPU -> dict of NumPy arrays (engines.run_gpu's keys).  Raises what the call raises."""
    from labelany3d_amd import fit_instances
    from labelany3d_amd.masks import fit_instances_bits, fit_instances_ex, fit_instances_poly, fit_instances_rle, pack_mask_bits, pack_polygons
    from labelany3d_amd.options import scheduling
    from oracle import la3d_oracle as O

    cache = {} if cache is None else cache
    np_ = lambda t: t.detach().cpu().numpy()   # noqa: E731

    def rles():
        if "rles" not in cache:
            cache["rles"] = [O.rle_encode(m) for m in c["masks"]]
        return cache["rles"]

    entry = r.get("entry")
    got = {}
    with scheduling(**{k: v for k, v in r.items() if k != "entry"}):
        kw = dict(ground=c["ground"], sample_idx=c["sidx"], image_index=c["image_index"], method="convex_hull")
        if entry == "rle":
            b, stg, aux = fit_instances_rle(c["depth"], rles(), c["K"], **kw)
        elif entry == "poly":
            b, stg, aux = fit_instances_poly(c["depth"], pack_polygons(c["segs"], c["H"], c["W"]), c["K"], **kw)
        elif entry == "bits":
            b, stg, aux = fit_instances_bits(c["depth"], pack_mask_bits(c["mb"]), c["K"], **kw)
        elif entry in EX_ENTRIES:
            hint, size, flt = E.ex_params(c, entry)
            src = dict(masks=c["mb"]) if entry == "ex_u8" else dict(rles=rles())
            res = fit_instances_ex(c["depth"], c["K"], filter=flt, image_size=size, area_hint=hint, **src, **kw)
            b, stg, aux = res["boxes"], res["status"], res["aux"]
            got.update(boxes2d=np_(res["boxes2d"]), stats=None if flt is None else np_(res["stats"]), flt=flt, size=size)
        else:
            b, stg, aux = fit_instances(c["depth"], c["mb"], c["K"], **kw)
        got.update(boxes=np_(b), status=np_(stg), aux=np_(aux))
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# the checker
# ------------------------------------------------------------------------------------------------------------------------------
def new_tally():
    z = lambda: dict(decided=0, tied=0, flat=0, fallback=0, rejected=0, refused={k: 0 for k in REASONS})   # noqa: E731
    return dict(full=z(), sample=z(), worst=0.0, n_pca_tie=0, n_filtered=0)


def expected_status(c, ref, r):
    """-> (status expected of run r, refusal reason per instance or None)."""
    why = [None] * c["B"]
    st = ref.st.copy()
    if c["full"]:
        for n in range(c["B"]):
            ok, why[n] = covered(c, n, r)
            if not ok:
                st[n] = 5
    assert (st >= 0).all(), "an instance some run fits has no oracle record"
    return st, why


def _ang(a, b):
    return np.abs((np.asarray(a) - b + np.pi) % (2 * np.pi) - np.pi)


def check_pin(want, got):
    """A pinned run against the default run: byte for byte."""
    return [f"{k} differs from the default run at {np.flatnonzero(~np.isclose(want[k], got[k], rtol=0, atol=0, equal_nan=True).reshape(len(want[k]), -1).all(1))[:5].tolist()}"
            for k in ("boxes", "status", "aux") if not np.array_equal(want[k], got[k], equal_nan=True)]


def check_run(c, ref, r, got, tally=None):
    """Compare one run's GPU output (run_gpu's dict) with ref = oracle_case(seed).  Returns the failures as strings (empty: the run
    agrees); tally (new_tally()) counts what was compared."""
    from oracle import la3d_oracle as O
    from tests.test_gpu_parity import assert_records, reference_axis_noise

    t = new_tally() if tally is None else tally
    tm = t["full" if c["full"] else "sample"]
    entry = r.get("entry")
    b, stg, aux = got["boxes"], got["status"], got["aux"]
    B = c["B"]
    nm = c["masks"].reshape(B, -1).sum(1)
    tag = f"seed {c['seed']} {c['H']}x{c['W']} B={B} P={c['P']} full={c['full']} {r}"
    st, why = expected_status(c, ref, r)
    if entry in EX_ENTRIES:
        b2d, stats, flt, size = got["boxes2d"], got["stats"], got["flt"], got["size"]
        if flt is not None:   # the fused filter: statistics and decisions against the oracle's; a dropped instance carries status 6 (the
            # filter comes first: it costs no passes)
            ref_stats = np.array([O.mask_stats(m, flt["boundary_threshold"]) for m in c["masks"]]).reshape(B, 4)
            keep = np.array([O.keep_instance(q, c["H"], True, flt["scale_threshold"]) for q in ref_stats], bool)
            if not np.array_equal(stats, ref_stats):
                return [f"fused filter: statistics differ at {np.flatnonzero((stats != ref_stats).any(1))[:4].tolist()}"]
            st = np.where(keep, st, 6).astype(np.int32)
            t["n_filtered"] += int((~keep).sum())
        okb = st == 0
        Kp = c["K"] if c["image_index"] is None else c["K"][c["image_index"]]
        with np.errstate(invalid="ignore", divide="ignore"):
            want2d = O.project_boxes(b, Kp if (c["P"] > 1 or c["image_index"] is not None) else c["K"][0], size)
        bad2d = np.flatnonzero(okb & ~(np.isclose(b2d, want2d, rtol=1e-12, atol=1e-9, equal_nan=True).all(1)))
        bad2d = [i for i in bad2d if np.isfinite(want2d[i]).all() and np.isfinite(b2d[i]).all()]
        if len(bad2d):
            return [f"2-D boxes of the epilogue differ at {bad2d[:4]}: {b2d[bad2d[0]]} vs {want2d[bad2d[0]]}"]
        if not np.isnan(b2d[st != 0]).all():
            return ["2-D boxes of a rejected / refused / filtered instance are not NaN"]
    if stg.tolist() != st.tolist():
        bad = np.flatnonzero(stg != st)
        return [f"status at {bad[:5].tolist()}: got {stg[bad][:5].tolist()} expected {st[bad][:5].tolist()} (mask kinds {[c['mkind'][i] for i in bad[:5]]}, "
                f"coverage {[why[i] for i in bad[:5]]}, active tiles {[active_tiles(c['masks'][i]) for i in bad[:5]]})"]
    ok = st == 0
    if not np.isnan(b[~ok]).all():
        return ["the record of a rejected / refused instance is not NaN: a box where the reference has none"]
    refused = st == 5
    # n_masked: exact wherever the call counted the mask - every instance but those refused by the frame, the ground row, the skew or
    # the active tiles, which leave before the count and report n_valid 0 and n_masked NaN (include/la3d.h); an instance refused for
    # its candidates has been through the fit stage and reports both exactly
    early = refused & np.array([w != "candidates" for w in why])
    late = refused & ~early
    if not np.array_equal(aux[~early, 2], nm[~early]):
        return [f"n_masked differs at {np.flatnonzero(~early & (aux[:, 2] != nm))[:5].tolist()}"]
    if not np.isnan(aux[early, 2]).all() or not (aux[early, 1] == 0).all():
        return [f"an instance refused before its mask was counted reports (n_valid, n_masked) = {aux[early, 1:3][:3].tolist()}, not (0, NaN)"]
    if not np.array_equal(aux[ok | late, 1], ref.nv[ok | late]):
        return [f"n_valid differs at {np.flatnonzero((ok | late) & (aux[:, 1] != ref.nv))[:5].tolist()}"]
    if not np.isnan(aux[refused, 0]).all() or not np.isnan(aux[refused, 3]).all():
        return ["a refused instance reports a yaw"]
    for n in np.flatnonzero(refused):
        tm["refused"][why[n]] += 1
    tm["rejected"] += int(((st != 0) & ~refused & (st != 6)).sum())
    fails = []
    for n in np.flatnonzero(ok):
        cls, rec = ref.cls[n], ref.rec[n]
        by_hull = aux[n, 3] < 0
        try:
            if cls == "decided":
                assert by_hull and aux[n, 3] <= -3, f"decided by the reference's hull, aux[3] = {aux[n, 3]}"
                assert_records(b[n:n + 1], rec[None], tag)
                t["worst"] = max(t["worst"], float(np.abs(b[n, :6] - rec[:6]).max() / max(np.abs(rec[:6]).max(), 1.0)))
            elif cls == "tied":
                assert by_hull and aux[n, 3] <= -3, f"decided by the reference's hull (tied edges), aux[3] = {aux[n, 3]}"
                near = ref.near[n]
                d = _ang(ref.table[n][0][near], aux[n, 0])
                i = int(near[np.argmin(d)])
                assert d.min() <= 1e-9, f"yaw {aux[n, 0]!r} is the yaw of no minimum-area edge (nearest: {ref.table[n][0][i]!r}, of {len(near)})"
                assert_records(b[n:n + 1], ref.box_under(n, ref.table[n][0][i])[None], tag)
            else:
                ext = max(np.abs(rec[3:6]).max(), 1e-300)
                assert abs(b[n, 4] - rec[4]) <= 1e-9 * max(ext, 1.0), f"height {b[n, 4]!r} vs {rec[4]!r}"
                assert abs(b[n, 1] - rec[1]) <= 1e-9 * max(ext, abs(rec[1]), 1.0), f"center y {b[n, 1]!r} vs {rec[1]!r}"
                if cls == "flat":                       # (the existing flat rule, oracle/campaigns/points.py: neither footprint has an area)
                    assert b[n, 3] * b[n, 5] <= 1e-9 * ext * ext, f"footprint dz x dx {b[n, 3] * b[n, 5]!r} of a flat cloud (extent {ext!r})"
                if cls == "fallback" and not by_hull:   # both sides took the PCA axis: the PCA rule (engines.check_run)
                    if aux[n, 3] >= 1e-9:
                        noise = reference_axis_noise(ref.kap[n:n + 1], aux[n:n + 1, 1], aux[n:n + 1, 3])
                        assert_records(b[n:n + 1], rec[None], tag, gap=aux[n:n + 1, 3], noise=noise)
                    else:
                        t["n_pca_tie"] += 1
            tm[cls] += 1
        except AssertionError as e:
            what = [ln for ln in str(e).splitlines() if ln.strip()]
            key = [ln for ln in what if "center" in ln or "R_cam" in ln or "vertices" in ln or "yaw" in ln or "aux[3]" in ln or "height" in ln or "footprint" in ln]
            p_ = plane_of(c, n)
            fails.append(f"record {n} ({cls}): {(key or what or ['mismatch'])[0].strip()}; mask kind {c['mkind'][n]} depth kind {c['dkind'][p_]} "
                         f"n_valid {int(aux[n, 1])} aux[3] {aux[n, 3]:.3g} | d center/dims {np.abs(b[n, :6] - rec[:6]).max():.3g} "
                         f"(scale {np.abs(rec[:6]).max():.3g}) dR {np.abs(b[n, 6:15] - rec[6:15]).max():.3g} yaw {aux[n, 0]!r} vs {ref.yaw[n]!r}")
    return fails


def tally_lines(t):
    out = []
    for mode in ("full", "sample"):
        m = t[mode]
        out.append(f"{'full-mask' if mode == 'full' else 'subsample'} mode: decided {m['decided']}, tied {m['tied']}, flat {m['flat']}, fallback {m['fallback']}, "
                   f"rejected by the reference's own rules {m['rejected']}, refused " + ", ".join(f"{k} {v}" for k, v in m["refused"].items()))
    out.append(f"worst relative error of center / dims among decided records: {t['worst']:.2e}; PCA fallbacks with an unresolved axis: "
               f"{t['n_pca_tie']}; dropped by the fused filter: {t['n_filtered']}")
    return out
