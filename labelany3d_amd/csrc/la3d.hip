// la3d.hip — the C-ABI of la3d_fit_instances* and its dispatcher (MI355X, gfx950 / CDNA4): the LabelAny3D geometric hot path -
// pinhole back-projection of masked depth pixels -> per-object moments -> closed-form PCA yaw -> extents along the principal
// axes -> 39-double box record.
//
// Reference semantics (behaviour only; nothing is copied):
//   depth_to_points   /root/reference/src/util.py:52-75
//   estimate_bbox     /root/reference/src/util_3dbox.py:106-178   (+ helpers :20-103, PCA yaw :181-186)
//
// Memory-bound integer/byte + fp64 reduction work: no MFMA.  Layout, kernel design and measurements: DESIGN.md.  Round 6 split the
// former 3 000-line file by engine, one translation unit each (compiled side by side):
//   la3d_instance.hip   one workgroup per instance: every call the others do not take (fit_instances_kernel)
//   la3d_rows.hip       up to sixteen workgroups per instance, one per band of rows: un-grounded u8 batches up to 160 instances
//   la3d_band.hip       two / four / eight workgroups per instance that meet through the workspace: grounded u8 batches of 1..160
//   la3d_split.hip      scan -> plan -> walk -> axis -> walk -> final over tile ranges: grounded run-length / polygon batches up to 160
//   la3d_walks.hpp      the walks over an instance's pixels (generic, tiled two-pass, separable single pass)
//   la3d_stages.hpp     moments -> axis, extents -> record, the in-kernel launch order, the culling plan, workgroup hand-off primitives
//   la3d_points.hip     explicit point clouds (la3d_fit_points) and the host-pointer single calls
//   la3d_masks.hip      whole-frame depth_to_points, mask decode / statistics;  la3d_consumers.hip  box consumers, depth statistics, matcher geometry
//   la3d_json.cpp       the host-side writer of 3dbbox.json + the build identity
// This file: the process defaults read once from the environment (config), workspace sizing, argument checks (fit_dispatch), and
// which engine fits a call (choose_engine; profiles/r06/r06_engines_by_batch.txt has the row in which each engine is the fastest).
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "la3d_device.hpp"
#include "la3d_poly.hpp"
#include "la3d_engines.hpp"
#include "la3d_hull.hpp"

namespace la3d {
thread_local char g_err[256] = "";

// ==========================================================================================
// Which engine fits a call.  Each engine says which calls its kernels can take (*_applies, la3d_engines.hpp); the batch
// limits below and the pins are applied here only.
// ==========================================================================================
// Row engine: by default batches of up to LA3D_ROWS_MAXB = ROWS_MAXB instances (0: never).  Small batches of u8 planes without a
// ground array: the single pass split over up to sixteen workgroups per instance, one per band of rows (B = 1 / 16 / 64 / 128:
// 18.2 / 19.3 / 24.0 / 30.0 us per call, profiles/r05/r05_rows_engine.txt); above, one workgroup per instance is as fast (round 6,
// us per call, instance | rows: B = 128: 37.1 | 30.3; 192: 39.8 | 41.1 - profiles/r06/r06_rows_engine.txt).
constexpr int ROWS_MAXB = 160;
// Band engine: by default the calls of 1 <= B <= BAND_MAXB instances (B >= 1 always holds here: a call of B = 0 returns before).
// Round 6: eight bands per instance put it ahead of the split engine from one instance on - B = 1 / 16 / 64: 23 / 28 / 34 us vs
// 32 / 36 / 43 (rounds 4-5 it took batches from 16 instances on) -, and above ~160 one workgroup per instance is as fast or
// faster: B = 192: 57 vs 54 us.  History - round 4, us per call, split | four bands once the band launch lost its memset: B = 1:
// 32.2 | 32.3; 16: 34.9 | 33.9; 64: 42.1 | 36.6; instance | two | four bands: B = 256: 59.7 | 58.6 | 60.0; 384: 63.4 | 66.2 | 78.1.
constexpr int BAND_MAXB = 160;
// Split engine: by default batches of up to SPLIT_MAXB instances, for every mask format.  Measured on MI355X, round 3 (BASELINE
// config-2 inputs, us per call, split vs one workgroup per instance; profiles/r03/r03_small_batches.txt): u8 planes B = 1 / 16 / 64 /
// 128 / 192 / 272 / 288 / 304 / 336: 34 / 37 / 45 / 50 / 58 / 70 / 74 / 76 / 81 vs 40 / 52 / 57 / 58 / 62 / 75 / 72 / 71 / 76; run
// lengths B = 1 / 16 / 64 / 160 / 256 / 288 / 304: 36 / 40 / 46 / 53 / 59 / 65 / 66 vs 47 / 57 / 59 / 66 / 64 / 66 / 65 (polygons
// ~1 us below both).  A lone 60-90 k-px instance keeps ONE CU's fp64 VALU busy for ~40 us in the instance engine; the split engine
// spreads its tiles over the chip at the price of six dependent launches.  Round 6: the crossover with the instance engine for
// grounded run lengths, split | instance: B = 128: 48 | 53, 192: 52.6 | 51.2, 256: 58 | 51; u8 planes up to 160 instances only
// (where the band engine does not apply: it is the faster one there) - grounded u8, split | instance: B = 192: 56.8 | 54.2, 256:
// 66.7 | 56.9 (profiles/r06/r06_engines_by_batch.txt).
constexpr int SPLIT_MAXB = 160;

// The engines are tried in the order rows -> band -> split -> instance.  pin (opt_engine, else LA3D_ENGINE) starts the walk at the
// pinned engine (rows2 counts as rows) and lifts that engine's batch limit; the instance engine takes every call.
//
// Round 5: a call WITHOUT a ground array on a frame the one-pass tile list covers, that the row engine does not take, takes the
// instance engine at EVERY batch size - its separable single pass (no pass B, no cull plan: a chain of three short phases per
// workgroup) is faster than the chain of six launches of the split engine and than the band engine's exchange from B = 1 on, for
// all three mask formats (profiles/r05/r05_small_batches.txt: B = 1 / 16 / 64 / 256, u8 planes: 27.7 / 32.1 / 36.8 / 45.1 us vs
// 31.7 / 34.8 / 37.9 / 59.8; run lengths 31.2 / 35.6 / 36.4 / 40.0 vs 34.3 / 37.9 / 43.3 / 57.4).  A skewed K (not separable) still
// takes this route - the kernel then runs its two passes -; a call WITH a ground array goes on to the band and split engines (two
// passes either way).  This shortcut belongs to the walk from rows: a pinned band or split engine skips it.
static int choose_engine(const FitParams& p, const CallFacts& f, int pin) {
  const int B = p.B, H = p.H, W = p.W;
  // a convex-hull call (la3d_fit_args::method) runs on the instance engine, whatever is pinned: pins change speed, never records
  if (f.method == LA3D_METHOD_CONVEX_HULL) return LA3D_ENGINE_INSTANCE;
  // masks given as bit planes: the instance engine at every batch size (the engines of several workgroups per instance have no
  // bit-plane form); pins give way, as for hull calls
  if (p.mask_bits != nullptr) return LA3D_ENGINE_INSTANCE;
  if (pin == LA3D_ENGINE_DEFAULT || pin == LA3D_ENGINE_ROWS || pin == LA3D_ENGINE_ROWS2) {
    if (rows_applies(p, f) && (pin != LA3D_ENGINE_DEFAULT || B <= config().rows_maxb)) return LA3D_ENGINE_ROWS;
    const bool single_pass_call = p.ground == nullptr && !f.sample && !p.sep_off && f.ldsmask && f.vec && W % 32 == 0 && W / 32 <= 255 &&
                                  (H + 7) / 8 <= 255 && ((W / 32) * ((H + 7) / 8) + NWAVE - 1) / NWAVE <= 256;
    if (single_pass_call) return LA3D_ENGINE_INSTANCE;
  }
  if (pin == LA3D_ENGINE_INSTANCE) return LA3D_ENGINE_INSTANCE;
  if (pin != LA3D_ENGINE_SPLIT && band_applies(p, f) && (pin == LA3D_ENGINE_BAND || B <= BAND_MAXB)) return LA3D_ENGINE_BAND;
  if (split_applies(p, f) && (pin == LA3D_ENGINE_SPLIT || B <= SPLIT_MAXB)) return LA3D_ENGINE_SPLIT;
  return LA3D_ENGINE_INSTANCE;
}

// the ONE place that reads the environment: a function-local static, initialised once (thread-safe since C++11)
const Config& config() {
  static const Config c = [] {
    Config k;
    const char* e = getenv("LA3D_ENGINE");
    k.engine = (e && !strcmp(e, "instance")) ? LA3D_ENGINE_INSTANCE : (e && !strcmp(e, "split")) ? LA3D_ENGINE_SPLIT
             : (e && !strcmp(e, "band")) ? LA3D_ENGINE_BAND : (e && !strcmp(e, "rows")) ? LA3D_ENGINE_ROWS
             : (e && !strcmp(e, "rows2")) ? LA3D_ENGINE_ROWS2 : LA3D_ENGINE_DEFAULT;
    e = getenv("LA3D_BANDS");
    k.bands = (e && (atoi(e) == 8 || atoi(e) == 4 || atoi(e) == 2)) ? atoi(e) : 0;
    e = getenv("LA3D_ROWS_MAXB");
    k.rows_maxb = e ? atoi(e) : ROWS_MAXB;
    e = getenv("LA3D_ROWS_WGS");          // workgroups the row engine spreads a batch over, at most
    k.rows_wgs = (e && atoi(e) > 0) ? atoi(e) : 640;
    e = getenv("LA3D_BALANCE");
    k.balance = !(e && e[0] == '0');
    e = getenv("LA3D_BUILD");             // plain | nocull -> LA3D_BUILD_PLAIN / LA3D_BUILD_NOCULL for every call
    k.build = (e && !strcmp(e, "plain")) ? LA3D_BUILD_PLAIN : (e && !strcmp(e, "nocull")) ? LA3D_BUILD_NOCULL : LA3D_BUILD_DEFAULT;
    e = getenv("LA3D_CULL_MIN");          // pass-B culling threshold (active tiles) for every input; unset: 224, u8 planes LA3D_CULL_MIN_U8
    k.cull_min = e ? atoi(e) : 0;
    e = getenv("LA3D_CULL_MIN_U8");
    k.cull_min_u8 = (e && atoi(e) > 0) ? atoi(e) : 128;
    e = getenv("LA3D_ORDER_SELF");        // 0: helper kernel in front of every ordered launch; 2: test mode of the fallback
    k.order_self = e ? atoi(e) : 1;
    e = getenv("LA3D_STAGGER_US");
    k.stagger_us = e ? atof(e) : -1.0;
    e = getenv("LA3D_BAND_TEST");
    k.band_test = e ? atoi(e) : 0;
    e = getenv("LA3D_SEP");               // 0: no separable single pass (the two-pass plain build everywhere)
    k.sep = !(e && e[0] == '0');
    return k;
  }();
  return c;
}
}

using namespace la3d;


// ==========================================================================================
// C-ABI
// ==========================================================================================
extern "C" {

int la3d_version(void) { return LA3D_ABI_VERSION; }

const char* la3d_last_error(void) { return g_err; }

double la3d_f16_round_host(double x) { return f16_round(x); }


// Workspace layout (one per concurrently running call; contents need not be initialised or preserved):
//   instance engine: [B] u32 sort keys of the size-balanced launch order (4*B bytes)
//   band engine:     [B] u32 sort keys | [B][4] u64 tagged arrival words | [B][BAND_NB_MAX = 8][22] f64 exchange records
//                    (band_workspace_bytes)
//   split engine:    [B][GEO_D] f64 geometry, then bit images, tile lists and partial-sum slots (split_workspace_bytes)
//   row engine:      [B][nb][ROWS_PART_D = 20] f64 partial records | [B][nb][2 W] u32 per-column depth ranges | [B] u64 tagged
//                    arrival words of the one-launch form; nb <= 16 bands per instance (rows_plan, rows_workspace_bytes)
size_t la3d_workspace_bytes(int B, int H, int W) {
  if (B <= 0) return 0;
  const size_t inst = (size_t)B * GEO_D * sizeof(double);  // kept as the minimum (older callers size by it)
  const size_t split = split_workspace_bytes(B, H, W);     // split engine: + bit image, tile lists, partial slots
  const size_t band = band_frame_ok(H, W, 2) ? band_workspace_bytes(B) : 0;   // band engine: keys, arrival words, exchange records
  const size_t rows = rows_workspace_bytes(B, H, W);         // row engine: partial records and per-column ranges of every band
  size_t m = split > inst ? split : inst;
  if (band > m) m = band;
  return rows > m ? rows : m;
}

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// The workspace of ONE call: la3d_workspace_bytes(B,H,W) for a PCA call; a convex-hull call adds its hand-off area behind that,
// 256-aligned - per instance the larger of the two modes' slots (hull_stride_bytes), so the size does not depend on sample_idx
size_t la3d_fit_workspace_bytes(const la3d_fit_args* args) {
  if (!fit_args_size_ok(args) || args->B <= 0) return 0;
  const size_t base = la3d_workspace_bytes(args->B, args->H, args->W);
  const bool has_method = (size_t)args->struct_size >= offsetof(la3d_fit_args, method) + sizeof(int32_t);
  if (!has_method || args->method != LA3D_METHOD_CONVEX_HULL) return base;
  const size_t full = hull_stride_bytes(false, args->W > 0 ? args->W : 0), samp = hull_stride_bytes(true, 0);
  return up256(base) + (size_t)args->B * (full > samp ? full : samp);
}

// la3d_fit_instances_bits' own arguments; offsets: the per-instance plane offsets of la3d_fit_instances_frames_bits (plane_stride is then 0)
struct BitsSource { const uint32_t* planes; int64_t plane_stride; int32_t flags; const int64_t* offsets = nullptr; };
struct FramesSource { const la3d_frame* rows; int32_t P; };                           // la3d_fit_instances_frames' own arguments
struct Depth16Source { const la3d_depth16* d; };                                      // la3d_fit_instances_depth16's own argument (checked there)

// Every fit entry ends here with its arguments in one block.  filter_on: the fused instance filter runs (the *_filtered entries
// always; the entries that take a block when block_filter_on says so).  who: the entry named in la3d_last_error().
// bs: the bit planes of la3d_fit_instances_bits (an internal parameter: the public block is frozen), null for every other entry.
// fr: the frame table of la3d_fit_instances_frames (H, W of the block are then bounds), null for every other entry.
// ds: the 16-bit depth planes of la3d_fit_instances_depth16 (a.depth is then null), null for every other entry but
// la3d_fit_instances_frames_depth16, which gives fr AND ds: the frame rows then count their depth_offset in 16-bit elements.
// la3d_fit_instances_frames_bits gives bs (with its offsets) AND fr, and ds for 16-bit planes.
static int fit_dispatch(const la3d_fit_args& a, bool filter_on, const char* who, const BitsSource* bs = nullptr,
                        const FramesSource* fr = nullptr, const Depth16Source* ds = nullptr) {
  const int B = a.B;
  int H = a.H, W = a.W;
  if (fr && H > 0 && W > 0 && W <= (1 << 20)) {
    // frames of different sizes: what the call reserves (LDS bit image, tile list) is sized for the bounds with the pitch rounded up
    // to whole words and, so that every frame inside the contract has a tiled form, for at least 64 tiles of 32 x 8 pixels
    W = (W + 31) / 32 * 32;
    const int ntx = W / 32, need = (64 + ntx - 1) / ntx;
    if ((H + 7) / 8 < need) H = need * 8;
  }
  const bool rle = a.rle_counts != nullptr || a.poly_xy != nullptr || bs != nullptr;   // "no u8 plane": the mask is decoded into the LDS bit image
  if ((!a.depth && !ds) || (!a.mask && !rle) || (a.rle_counts && !a.rle_offsets) || (a.poly_xy && (!a.ring_offsets || !a.inst_rings)) ||
      !a.K || !a.out || !a.status || B < 0 || H <= 0 || W <= 0 ||
      a.depth_plane_stride < 0 || (a.k_stride != 0 && a.k_stride < 9) || (long long)H * W > (1LL << 28))
    return refuse(who, "bad argument");
  if (a.method != LA3D_METHOD_PCA && a.method != LA3D_METHOD_CONVEX_HULL) return refuse(who, "unknown method (LA3D_METHOD_PCA or LA3D_METHOD_CONVEX_HULL)");
  if (B == 0) return LA3D_SUCCESS;
  if (!a.workspace || (reinterpret_cast<uintptr_t>(a.workspace) & 7))
    return refuse(who, a.method == LA3D_METHOD_CONVEX_HULL ? "a convex-hull call needs a workspace of la3d_fit_workspace_bytes() bytes (8-aligned)"
                                                           : "workspace of la3d_workspace_bytes() bytes (8-aligned) required");
  FitParams p;   // (every other field keeps its default: see FitParams)
  p.geo = static_cast<double*>(a.workspace);
  p.depth = a.depth; p.depth_plane_stride = ds ? ds->d->plane_stride : a.depth_plane_stride; p.image_index = a.image_index;
  p.mask = a.mask; p.K = a.K; p.k_stride = a.k_stride; p.ground = a.ground; p.sample_idx = a.sample_idx;
  p.rle_counts = a.rle_counts; p.rle_offsets = reinterpret_cast<const long long*>(a.rle_offsets);
  p.poly_xy = a.poly_xy;
  p.poly_ring_off = reinterpret_cast<const long long*>(a.ring_offsets);
  p.poly_inst_rings = reinterpret_cast<const long long*>(a.inst_rings);
  if (bs) {
    p.mask_bits = bs->planes; p.bits_plane_stride = bs->plane_stride;
    p.bits_vec = ((reinterpret_cast<uintptr_t>(bs->planes) & 15) == 0 && bs->plane_stride % 4 == 0) ? 1 : 0;
    p.bits_span = (bs->flags & LA3D_BITS_HEIGHT_SPAN) ? 1 : 0;
    p.bits_offsets = reinterpret_cast<const long long*>(bs->offsets);
  }
  p.B = B; p.H = H; p.W = W; p.HW = H * W;
  p.nwords = (p.HW + 31) / 32;
  p.rows_aligned = (W % 4 == 0);
  p.rcpW = 1.0f / (float)W;
  p.out = a.out; p.status = a.status; p.aux = a.aux;
  p.band_test = config().band_test;
  // build of the call: the default (separable single pass where it applies), PLAIN = the two-pass form for every camera, NOCULL = the
  // two-pass form that also walks EVERY active tile in pass B (no culling plan): the reference build the culling tests compare with
  const int build = a.opt_build != LA3D_BUILD_DEFAULT ? a.opt_build : config().build;
  p.sep_off = (config().sep == 0 || build != LA3D_BUILD_DEFAULT) ? 1 : 0;
  p.cull_min = build == LA3D_BUILD_NOCULL ? 0x7fffffff : config().cull_min > 0 ? config().cull_min : (a.mask != nullptr ? config().cull_min_u8 : CULL_MIN);
  p.proj = a.proj; p.proj_w = a.image_width; p.proj_h = a.image_height;
  p.area_hint = a.area_hint;
  p.opt_engine = a.opt_engine; p.opt_order = a.opt_launch_order; p.opt_build = a.opt_build;
  p.frame_w = W;
  if (fr) { p.frames = fr->rows; p.frames_P = fr->P; p.frames_max_h = a.H; p.frames_max_w = a.W; }
  if (a.frame_width != 0 && a.frame_width != W) {
    // rows padded on the right (la3d_fit_args::frame_width): run-length / polygon masks, word-aligned rows
    if (a.frame_width < 0 || a.frame_width > W || a.mask != nullptr || W % 32 != 0)
      return refuse(who, bs ? "frame_width must be 0 or in (0, W], with W % 32 == 0"
                            : "frame_width must be 0 or in (0, W], with run-length / polygon masks and W % 32 == 0");
    p.frame_w = a.frame_width;
  }
  if (filter_on) {
    if (!rle || a.filter_boundary < 0) return refuse(who, "the fused filter needs run-length or polygon masks and boundary >= 0");
    p.filter_boundary = a.filter_boundary; p.filter_min_area = a.filter_min_area; p.filter_max_edge = a.filter_max_edge;
    p.filter_stats = a.stats;
  }
  const int bit_bytes = mask_bit_bytes(p.HW);
  CallFacts f;
  f.ldsmask = bit_bytes <= MAX_MASK_LDS;
  p.mask_lds_bytes = f.ldsmask ? bit_bytes : 0;
  if (rle && !f.ldsmask) return refuse(who, bs ? "bit-plane masks need the bit image in LDS (H*W <= 1048576)"
                          : "run-length / polygon masks need the bit image in LDS (H*W <= 1048576)", LA3D_ERR_UNSUPPORTED);
  // 16-byte vector path: every plane base 16-aligned (the u8 mask only when it is read at all)
  // (16-bit planes: a lane's quad is 8 bytes - base 8-aligned, stride a multiple of four elements)
  f.vec = (p.HW % 16 == 0) && (rle || (reinterpret_cast<uintptr_t>(a.mask) & 15) == 0) &&
          (ds ? (reinterpret_cast<uintptr_t>(ds->d->planes) & 7) == 0 : (reinterpret_cast<uintptr_t>(a.depth) & 15) == 0) &&
          (p.depth_plane_stride % 4 == 0);
  f.sample = a.sample_idx != nullptr;
  f.method = a.method;
  f.frames = fr != nullptr;
  if (a.method == LA3D_METHOD_CONVEX_HULL)
    f.hull_area = static_cast<unsigned char*>(a.workspace) + up256(la3d_workspace_bytes(B, H, W));
  f.lds = (size_t)p.mask_lds_bytes + sizeof(Shared);
  // polygons: the side stage sits behind Shared, where the tile list / rank prefix go later (disjoint in time)
  f.poly_stage = a.poly_xy ? (size_t)POLY_STAGE_BYTES : 0;
  const int pin = a.opt_engine != LA3D_ENGINE_DEFAULT ? a.opt_engine : config().engine;   // per-call pin, else the process default
  hipStream_t s = static_cast<hipStream_t>(a.stream);
  // frames of different sizes: the instance engine at every batch size (no other engine reads a frame table); pins give way
  if (fr && !ds) return instance_fit(p, f, s, a.workspace, who);
  if (ds) {
    // 16-bit depth planes: the instance engine at every batch size (no other engine has a 16-bit form); pins give way
    // (with a frame table - la3d_fit_instances_frames_depth16 - the 16-bit units launch their FRAMES instantiations: f.frames)
    FitParams16 q;
    static_cast<FitParams&>(q) = p;
    q.depth16 = static_cast<const unsigned short*>(ds->d->planes);
    q.d16_scale = ds->d->scale;
    q.d16_hole = (ds->d->flags & LA3D_DEPTH_ZERO_IS_HOLE) ? 1 : 0;
    return ds->d->dtype == LA3D_DTYPE_F16 ? instance_fit_f16(q, f, s, a.workspace, who) : instance_fit_u16(q, f, s, a.workspace, who);
  }
  switch (choose_engine(p, f, pin)) {
  case LA3D_ENGINE_ROWS:   // (two launches when pinned so, and for a call captured into a HIP graph: it would replay with the same tag)
    return rows_fit(p, pin == LA3D_ENGINE_ROWS2 || stream_capturing(s), s, a.workspace);
  case LA3D_ENGINE_BAND:
    return band_fit(p, s, a.workspace);
  case LA3D_ENGINE_SPLIT: {
    const int rc = split_fit(p, a.workspace, s);   // (the split engine's final kernel does not project: one small follow-up launch)
    if (rc != LA3D_SUCCESS || !p.proj) return rc;
    return la3d_project_boxes(a.out, a.K, a.k_stride, a.image_index, B, p.proj_w, p.proj_h, p.proj, a.stream);   // (la3d_consumers.hip)
  }
  default:
    return instance_fit(p, f, s, a.workspace, who);
  }
}

// The entries of ABI 1 fill a zeroed block (no filter, no options) and keep their own checks and error texts.
static la3d_fit_args legacy_args(const float* depth, int64_t depth_plane_stride, const int32_t* image_index, const double* K,
                                 int32_t k_stride, const double* ground, const int32_t* sample_idx, int B, int H, int W,
                                 double* out, int32_t* status, double* aux, void* workspace, void* stream) {
  la3d_fit_args a{};
  a.struct_size = (int32_t)sizeof(a);
  a.B = B; a.H = H; a.W = W;
  a.depth = depth; a.depth_plane_stride = depth_plane_stride; a.image_index = image_index;
  a.K = K; a.k_stride = k_stride; a.ground = ground; a.sample_idx = sample_idx;
  a.out = out; a.status = status; a.aux = aux; a.workspace = workspace; a.stream = stream;
  return a;
}

// polygon parts of the legacy entries: a batch of zero instances may come without vertices (an empty array has no data pointer) and
// is still a polygon call - poly_xy then borrows ring_offsets' non-null value, which nothing reads
static void legacy_poly(la3d_fit_args& a, const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings) {
  a.poly_xy = poly_xy ? poly_xy : reinterpret_cast<const int32_t*>(ring_offsets);
  a.ring_offsets = ring_offsets; a.inst_rings = inst_rings;
}

static void legacy_filter(la3d_fit_args& a, int boundary, int min_area, int max_edge, int32_t* stats) {
  a.filter_boundary = boundary; a.filter_min_area = min_area; a.filter_max_edge = max_edge; a.stats = stats;
}

int la3d_fit_instances(const float* depth, int64_t depth_plane_stride, const int32_t* image_index,
                       const uint8_t* mask, const double* K, int32_t k_stride, const double* ground,
                       const int32_t* sample_idx, int B, int H, int W, double* out, int32_t* status, double* aux,
                       void* workspace, void* stream) {
  la3d_fit_args a = legacy_args(depth, depth_plane_stride, image_index, K, k_stride, ground, sample_idx, B, H, W, out, status, aux,
                                workspace, stream);
  a.mask = mask;
  return fit_dispatch(a, false, "la3d_fit_instances");
}

int la3d_fit_instances_rle(const float* depth, int64_t depth_plane_stride, const int32_t* image_index,
                           const int32_t* rle_counts, const int64_t* rle_offsets, const double* K, int32_t k_stride,
                           const double* ground, const int32_t* sample_idx, int B, int H, int W, double* out,
                           int32_t* status, double* aux, void* workspace, void* stream) {
  if (!rle_counts && B > 0) return refuse("la3d_fit_instances_rle", "bad argument");
  la3d_fit_args a = legacy_args(depth, depth_plane_stride, image_index, K, k_stride, ground, sample_idx, B, H, W, out, status, aux,
                                workspace, stream);
  a.rle_counts = rle_counts; a.rle_offsets = rle_offsets;
  return fit_dispatch(a, false, "la3d_fit_instances_rle");
}

int la3d_fit_instances_poly(const float* depth, int64_t depth_plane_stride, const int32_t* image_index,
                            const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, const double* K,
                            int32_t k_stride, const double* ground, const int32_t* sample_idx, int B, int H, int W, double* out,
                            int32_t* status, double* aux, void* workspace, void* stream) {
  if ((!poly_xy || !ring_offsets || !inst_rings) && B > 0) return refuse("la3d_fit_instances_poly", "bad argument");
  la3d_fit_args a = legacy_args(depth, depth_plane_stride, image_index, K, k_stride, ground, sample_idx, B, H, W, out, status, aux,
                                workspace, stream);
  legacy_poly(a, poly_xy, ring_offsets, inst_rings);
  return fit_dispatch(a, false, "la3d_fit_instances_poly");
}

// The *_filtered entries always run the filter: boundary < 0 is an error, max_edge <= 0 drops every instance.
int la3d_fit_instances_rle_filtered(const float* depth, int64_t depth_plane_stride, const int32_t* image_index,
                                    const int32_t* rle_counts, const int64_t* rle_offsets, const double* K, int32_t k_stride,
                                    const double* ground, const int32_t* sample_idx, int B, int H, int W, int boundary,
                                    int min_area, int max_edge, double* out, int32_t* status, double* aux, int32_t* stats,
                                    void* workspace, void* stream) {
  if (!rle_counts && B > 0) return refuse("la3d_fit_instances_rle_filtered", "bad argument");
  la3d_fit_args a = legacy_args(depth, depth_plane_stride, image_index, K, k_stride, ground, sample_idx, B, H, W, out, status, aux,
                                workspace, stream);
  a.rle_counts = rle_counts; a.rle_offsets = rle_offsets;
  legacy_filter(a, boundary, min_area, max_edge, stats);
  return fit_dispatch(a, true, "la3d_fit_instances_rle_filtered");
}

int la3d_fit_instances_poly_filtered(const float* depth, int64_t depth_plane_stride, const int32_t* image_index,
                                     const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings,
                                     const double* K, int32_t k_stride, const double* ground, const int32_t* sample_idx, int B,
                                     int H, int W, int boundary, int min_area, int max_edge, double* out, int32_t* status,
                                     double* aux, int32_t* stats, void* workspace, void* stream) {
  if ((!poly_xy || !ring_offsets || !inst_rings) && B > 0) return refuse("la3d_fit_instances_poly_filtered", "bad argument");
  la3d_fit_args a = legacy_args(depth, depth_plane_stride, image_index, K, k_stride, ground, sample_idx, B, H, W, out, status, aux,
                                workspace, stream);
  legacy_poly(a, poly_xy, ring_offsets, inst_rings);
  legacy_filter(a, boundary, min_area, max_edge, stats);
  return fit_dispatch(a, true, "la3d_fit_instances_poly_filtered");
}

// what la3d_fit_instances_ex and la3d_fit_instances_bits check alike
static int check_block_options(const la3d_fit_args& a, const char* who) {
  if (a.proj && !(a.image_width > 0 && a.image_height > 0)) return refuse(who, "proj needs image_width / image_height > 0");
  if (a.opt_engine < 0 || a.opt_engine > LA3D_ENGINE_ROWS2 || a.opt_launch_order < 0 || a.opt_launch_order > LA3D_ORDER_ON ||
      a.opt_build < 0 || a.opt_build > LA3D_BUILD_NOCULL)
    return refuse(who, "bad opt_engine / opt_launch_order / opt_build");
  return LA3D_SUCCESS;
}

// Whether a block entry runs the fused filter: filter_boundary >= 0 AND filter_max_edge > 0.  A zero-initialised block (the natural
// C idiom, and what "missing fields are zero" gives) means NO filter - max_edge == 0 would reject every instance (edge < 0 never holds)
static bool block_filter_on(const la3d_fit_args& a) { return a.filter_boundary >= 0 && a.filter_max_edge > 0; }

int la3d_fit_instances_ex(const la3d_fit_args* args) {
  const char* who = "la3d_fit_instances_ex";
  if (!fit_args_size_ok(args)) return refuse(who, "bad struct_size");
  const la3d_fit_args a = fit_args_copy(args);
  const int kinds = (a.mask ? 1 : 0) + (a.rle_counts ? 1 : 0) + (a.poly_xy ? 1 : 0);
  if (kinds != 1 && a.B > 0) return refuse(who, "give exactly one of mask / rle_counts / poly_xy");
  if (a.poly_xy && (!a.ring_offsets || !a.inst_rings)) return refuse(who, "polygon masks need ring_offsets and inst_rings");
  const int rc = check_block_options(a, who);
  if (rc != LA3D_SUCCESS) return rc;
  return fit_dispatch(a, block_filter_on(a), who);
}

size_t la3d_mask_bits_words(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  return (size_t)(((long long)H * W + 31) / 32);
}

int la3d_fit_instances_bits(const la3d_fit_args* args, const uint32_t* mask_bits, int64_t bits_plane_stride, int32_t flags) {
  const char* who = "la3d_fit_instances_bits";
  if (!fit_args_size_ok(args)) return refuse(who, "bad struct_size");
  const la3d_fit_args a = fit_args_copy(args);
  if (a.mask || a.rle_counts || a.poly_xy) return refuse(who, "the masks are the bit planes - mask, rle_counts and poly_xy must be NULL");
  if (flags & ~(int32_t)LA3D_BITS_HEIGHT_SPAN) return refuse(who, "unknown flags (LA3D_BITS_HEIGHT_ROWS or LA3D_BITS_HEIGHT_SPAN)");
  if (a.B > 0 && (!mask_bits || (reinterpret_cast<uintptr_t>(mask_bits) & 3))) return refuse(who, "mask_bits must be a 4-byte aligned device pointer");
  if (a.B > 0 && a.H > 0 && a.W > 0 && bits_plane_stride < (int64_t)la3d_mask_bits_words(a.H, a.W))
    return refuse(who, "bits_plane_stride is smaller than la3d_mask_bits_words(H, W)");
  const int rc = check_block_options(a, who);
  if (rc != LA3D_SUCCESS) return rc;
  const BitsSource bs{mask_bits, bits_plane_stride, flags};
  return fit_dispatch(a, block_filter_on(a), who, &bs);
}

// what la3d_fit_instances_depth16 and la3d_fit_instances_frames_depth16 check alike, in two steps (the entry copies its block between
// them): the two blocks and the planes pointer, then the value rule of the la3d_depth16 block
static int depth16_block_head(const la3d_fit_args* args, const la3d_depth16* depth, const char* who) {
  static_assert(sizeof(la3d_depth16) == 32, "la3d_depth16 is part of the ABI");
  if (!fit_args_size_ok(args)) return refuse(who, "bad struct_size");
  if (!depth) return refuse(who, "depth (the la3d_depth16 block) is NULL");
  if (depth->struct_size < (int32_t)sizeof(la3d_depth16)) return refuse(who, "bad struct_size of la3d_depth16");
  if (depth->dtype != LA3D_DTYPE_F16 && depth->dtype != LA3D_DTYPE_U16) return refuse(who, "unknown dtype (LA3D_DTYPE_F16 or LA3D_DTYPE_U16)");
  if (!depth->planes || (reinterpret_cast<uintptr_t>(depth->planes) & 1)) return refuse(who, "planes must be a 2-byte aligned device pointer");
  return LA3D_SUCCESS;
}
static int depth16_block_values(const la3d_depth16* depth, const char* who) {
  if (depth->dtype == LA3D_DTYPE_U16) {
    if (!(depth->scale > 0.0f && depth->scale <= 3.4028234663852886e38f))   // (false for NaN)
      return refuse(who, "the scale of LA3D_DTYPE_U16 planes must be finite and > 0");
    if (depth->flags & ~(int32_t)LA3D_DEPTH_ZERO_IS_HOLE) return refuse(who, "unknown flags (LA3D_DEPTH_ZERO_IS_HOLE or 0)");
  } else if (depth->flags != 0) {
    return refuse(who, "flags must be 0 for LA3D_DTYPE_F16 planes");
  }
  return LA3D_SUCCESS;
}

int la3d_fit_instances_depth16(const la3d_fit_args* args, const la3d_depth16* depth, const uint32_t* mask_bits,
                               int64_t bits_plane_stride, int32_t bits_flags) {
  const char* who = "la3d_fit_instances_depth16";
  int rc = depth16_block_head(args, depth, who);
  if (rc != LA3D_SUCCESS) return rc;
  const la3d_fit_args a = fit_args_copy(args);
  if (a.depth || a.depth_plane_stride != 0)
    return refuse(who, "the depth planes come in the la3d_depth16 block - args->depth must be NULL and depth_plane_stride 0");
  rc = depth16_block_values(depth, who);
  if (rc != LA3D_SUCCESS) return rc;
  if (depth->plane_stride < 0 || (depth->plane_stride != 0 && a.H > 0 && a.W > 0 && depth->plane_stride < (int64_t)a.H * a.W))
    return refuse(who, "plane_stride must be 0 (one shared plane) or >= H*W elements");
  const int kinds = (a.mask ? 1 : 0) + (a.rle_counts ? 1 : 0) + (a.poly_xy ? 1 : 0) + (mask_bits ? 1 : 0);
  if (kinds != 1) return refuse(who, "give exactly one mask source: mask / rle_counts / poly_xy in the block, or mask_bits");
  if (a.poly_xy && (!a.ring_offsets || !a.inst_rings)) return refuse(who, "polygon masks need ring_offsets and inst_rings");
  // (the rules of la3d_fit_instances_bits, but for a source that is optional here: they hold for B = 0 too, and say bits_flags)
  if (mask_bits) {
    if (bits_flags & ~(int32_t)LA3D_BITS_HEIGHT_SPAN) return refuse(who, "unknown bits_flags (LA3D_BITS_HEIGHT_ROWS or LA3D_BITS_HEIGHT_SPAN)");
    if (reinterpret_cast<uintptr_t>(mask_bits) & 3) return refuse(who, "mask_bits must be a 4-byte aligned device pointer");
    if (a.B > 0 && a.H > 0 && a.W > 0 && bits_plane_stride < (int64_t)la3d_mask_bits_words(a.H, a.W))
      return refuse(who, "bits_plane_stride is smaller than la3d_mask_bits_words(H, W)");
  }
  rc = check_block_options(a, who);
  if (rc != LA3D_SUCCESS) return rc;
  const BitsSource bs{mask_bits, bits_plane_stride, bits_flags};
  const Depth16Source ds{depth};
  return fit_dispatch(a, block_filter_on(a), who, mask_bits ? &bs : nullptr, nullptr, &ds);
}

// what la3d_fit_instances_frames and la3d_fit_instances_frames_depth16 check alike on the copied block and the frame table
// (bits: la3d_fit_instances_frames_bits, whose masks are its own arguments - it has refused mask / rle_counts / poly_xy itself)
static int check_frames_call(const la3d_fit_args& a, const la3d_frame* frames, int32_t P, const char* who, bool bits = false) {
  static_assert(sizeof(la3d_frame) == 24, "la3d_frame is part of the ABI");
  if (a.mask) return refuse(who, "u8 mask planes are not supported - run lengths or polygon parts", LA3D_ERR_UNSUPPORTED);
  if (a.method == LA3D_METHOD_CONVEX_HULL) return refuse(who, "method = LA3D_METHOD_CONVEX_HULL is not supported in this form", LA3D_ERR_UNSUPPORTED);
  const int kinds = (a.rle_counts ? 1 : 0) + (a.poly_xy ? 1 : 0);
  if (!bits && kinds != 1 && a.B > 0) return refuse(who, "give exactly one of rle_counts / poly_xy");
  if (a.poly_xy && (!a.ring_offsets || !a.inst_rings)) return refuse(who, "polygon masks need ring_offsets and inst_rings");
  if (P < 0 || (a.B > 0 && (!frames || P == 0 || (reinterpret_cast<uintptr_t>(frames) & 7))))
    return refuse(who, "frames must be an 8-byte aligned device pointer to P >= 1 rows");
  if (a.B > 0 && !a.image_index) return refuse(who, "image_index is required (instance n belongs to frame row image_index[n])");
  if (a.depth_plane_stride != 0 || a.frame_width != 0)
    return refuse(who, "depth_plane_stride and frame_width must be 0 (the frame table holds them per image)");
  return LA3D_SUCCESS;
}

int la3d_fit_instances_frames(const la3d_fit_args* args, const la3d_frame* frames, int32_t P) {
  const char* who = "la3d_fit_instances_frames";
  if (!fit_args_size_ok(args)) return refuse(who, "bad struct_size");
  la3d_fit_args a = fit_args_copy(args);
  int rc = check_frames_call(a, frames, P, who);
  if (rc != LA3D_SUCCESS) return rc;
  if (reinterpret_cast<uintptr_t>(a.depth) & 15) return refuse(who, "depth must be 16-byte aligned");
  a.image_width = a.image_height = 1.0;   // (ignored: proj clamps to the instance's own frame)
  rc = check_block_options(a, who);
  if (rc != LA3D_SUCCESS) return rc;
  const FramesSource fs{frames, P};
  return fit_dispatch(a, block_filter_on(a), who, nullptr, &fs);
}

// the frames call on 16-bit planes: the checks of both parents, then fit_dispatch with both sources (it launches the FRAMES
// instantiations of the 16-bit units); depth_offset of the frame rows counts 16-bit ELEMENTS
int la3d_fit_instances_frames_depth16(const la3d_fit_args* args, const la3d_depth16* depth, const la3d_frame* frames, int32_t P) {
  const char* who = "la3d_fit_instances_frames_depth16";
  int rc = depth16_block_head(args, depth, who);
  if (rc != LA3D_SUCCESS) return rc;
  la3d_fit_args a = fit_args_copy(args);
  if (a.depth) return refuse(who, "the depth planes come in the la3d_depth16 block - args->depth must be NULL");
  rc = depth16_block_values(depth, who);
  if (rc != LA3D_SUCCESS) return rc;
  if (depth->plane_stride != 0) return refuse(who, "plane_stride of the la3d_depth16 block must be 0 (the frame table says where every plane lies)");
  rc = check_frames_call(a, frames, P, who);
  if (rc != LA3D_SUCCESS) return rc;
  if (reinterpret_cast<uintptr_t>(depth->planes) & 7) return refuse(who, "planes (the base of the ragged buffer) must be 8-byte aligned");
  a.image_width = a.image_height = 1.0;   // (ignored: proj clamps to the instance's own frame)
  rc = check_block_options(a, who);
  if (rc != LA3D_SUCCESS) return rc;
  const FramesSource fs{frames, P};
  const Depth16Source ds{depth};
  return fit_dispatch(a, block_filter_on(a), who, nullptr, &fs, &ds);
}

// the frames call on bit planes, one plane per instance at its own offset: the checks of la3d_fit_instances_frames (with depth16: of
// la3d_fit_instances_frames_depth16) and of la3d_fit_instances_bits, then fit_dispatch with the sources of both
int la3d_fit_instances_frames_bits(const la3d_fit_args* args, const la3d_depth16* depth16, const la3d_frame* frames, int32_t P,
                                   const uint32_t* mask_bits, const int64_t* bits_offsets, int32_t bits_flags) {
  const char* who = "la3d_fit_instances_frames_bits";
  int rc = LA3D_SUCCESS;
  if (depth16) {
    rc = depth16_block_head(args, depth16, who);
    if (rc != LA3D_SUCCESS) return rc;
  } else if (!fit_args_size_ok(args)) {
    return refuse(who, "bad struct_size");
  }
  la3d_fit_args a = fit_args_copy(args);
  if (depth16) {
    if (a.depth) return refuse(who, "the depth planes come in the la3d_depth16 block - args->depth must be NULL");
    rc = depth16_block_values(depth16, who);
    if (rc != LA3D_SUCCESS) return rc;
    if (depth16->plane_stride != 0) return refuse(who, "plane_stride of the la3d_depth16 block must be 0 (the frame table says where every plane lies)");
  }
  if (a.mask || a.rle_counts || a.poly_xy) return refuse(who, "the masks are the bit planes - mask, rle_counts and poly_xy must be NULL");
  if (bits_flags & ~(int32_t)LA3D_BITS_HEIGHT_SPAN) return refuse(who, "unknown bits_flags (LA3D_BITS_HEIGHT_ROWS or LA3D_BITS_HEIGHT_SPAN)");
  rc = check_frames_call(a, frames, P, who, true);
  if (rc != LA3D_SUCCESS) return rc;
  // (one plane per instance at its own offset, read in 16-byte groups: no stride to check, and a stricter alignment than the uniform form's)
  if (a.B > 0 && (!mask_bits || (reinterpret_cast<uintptr_t>(mask_bits) & 15))) return refuse(who, "mask_bits must be a 16-byte aligned device pointer");
  if (a.B > 0 && (!bits_offsets || (reinterpret_cast<uintptr_t>(bits_offsets) & 7)))
    return refuse(who, "bits_offsets must be an 8-byte aligned device pointer to B plane offsets");
  if (depth16 ? (reinterpret_cast<uintptr_t>(depth16->planes) & 7) != 0 : (reinterpret_cast<uintptr_t>(a.depth) & 15) != 0)
    return refuse(who, depth16 ? "planes (the base of the ragged buffer) must be 8-byte aligned" : "depth must be 16-byte aligned");
  a.image_width = a.image_height = 1.0;   // (ignored: proj clamps to the instance's own frame)
  rc = check_block_options(a, who);
  if (rc != LA3D_SUCCESS) return rc;
  const BitsSource bs{mask_bits, 0, bits_flags, bits_offsets};
  const FramesSource fs{frames, P};
  const Depth16Source ds{depth16};
  return fit_dispatch(a, block_filter_on(a), who, &bs, &fs, depth16 ? &ds : nullptr);
}

}  // extern "C"
