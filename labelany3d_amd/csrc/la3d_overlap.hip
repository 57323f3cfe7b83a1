// la3d_overlap.hip - mask overlap on bit planes (include/la3d.h "mask overlap on bit planes"): what relates two planes of one image,
//     inter[g][i, j] = popcount(A_i & B_j)        for the rows i of A and j of B of every group g (an image),
// the planes' own areas from the same loads, the ratios by kind, and the greedy mask NMS that reads a self overlap.
//   plan (host)       the tile table: one row per workgroup - up to 8 x 8 planes of one group and a range of words.  A call with few
//                     tiles gets the word range split into chunks, so that one image still fills the chip.
//   overlap           a register-tiled "bit GEMM": each lane loads 16 bytes of each of the 8 + 8 planes at its own word position and
//                     keeps 64 + 16 int counters (and + popcount-accumulate: 2 instructions per 32 pixel pairs); no LDS staging of the
//                     planes.  The counters are folded across the wave by DPP (a transposing butterfly over xor 1 / xor 2, then row
//                     rotations: 80 values cost what five plain wave sums would), the 16 row sums of the workgroup meet in LDS, and
//                     the tile's 80 ints go to its own slot of the workspace.
//   finish            one workgroup per tile sums the chunks' slots and writes inter, the areas and the ratio - every element has one
//                     writer, no atomics, nothing to pre-clear.
//   nms               one workgroup per group walks the rows in the given order; lanes work over the later rows.
// Frames form: the geometry of a group comes from its la3d_frame row, and every row of planes is checked on the device before an
// address is formed from it; a refused row reads nothing and gets -1 / NaN (the pattern of la3d_open_bits_frames).
#include <cstdint>
#include <cstddef>
#include <cstring>

#include "la3d_bitplanes.hpp"   // (at, plane_offset_ok)

namespace {
constexpr int OT = 256;                  // threads of an overlap workgroup
constexpr int TILE = 8;                  // planes per side of a tile
constexpr int STEP = OT * 4;             // words of every plane a workgroup takes per step: 16 bytes per lane
constexpr int SLOT = TILE * TILE + 2 * TILE;   // ints a tile leaves in the workspace: 64 pair counts, 8 areas of A, 8 areas of B
constexpr int WANT_WGS = 1024;           // workgroups a call is spread over where its planes allow: four per CU
constexpr long long MAX_WORDS = 1LL << 23;     // H * W_stored <= 2^28: a count fits int32
constexpr long long MAX_PAIRS = 0x7fffffffLL;
constexpr int NMS_T = 256;
constexpr int NMS_MAX = 46340;           // rows of a group: floor(sqrt(2^31 - 1))
constexpr int DPP_ROR4 = 0x124, DPP_ROR8 = 0x128;   // row_ror: lane l of a 16-lane row reads lane (l - n) & 15 of it

struct OverlapParams {
  const unsigned* a; const unsigned* b;
  long long a_stride, b_stride;
  const long long* a_off; const long long* b_off;
  const int* a_img; const int* b_img;
  long long a_words, b_words;
  const la3d_frame* frames; int P, H, W;
  const la3d_overlap_tile* tiles;
  int* partial;
  int* inter; int* area_a; int* area_b; double* iou; int kind;
};

// frames form: the group's frame row keeps the la3d_frame contract (the check of the fit) and its words are those the plan split
template <bool FRAMES>
__device__ inline bool group_ok(const OverlapParams& p, const la3d_overlap_tile& t) {
  if constexpr (FRAMES) {
    if ((unsigned)t.g >= (unsigned)p.P) return false;
    const FrameRow r = frame_row_load(p.frames + t.g);
    if (!frame_row_ok(r, p.H, p.W)) return false;
    return (int)(((long long)r.H * r.W) >> 5) == t.nw;
  }
  return true;
}
// the words from the side's base to the plane of row `row` (counted over the call), or -1: refused (frames form) - image index,
// offset, end of the plane, each before an address is formed
template <bool FRAMES>
__device__ inline long long plane_at(long long stride, const long long* off, const int* img, long long words, int row, int g, int nw) {
  if constexpr (FRAMES) {
    if (img[row] != g) return -1;
    const long long o = off[row];
    if (!plane_offset_ok(o) || o > words - nw) return -1;
    return o;
  }
  return (long long)row * stride;
}

// the four words of one plane a lane takes in the step that starts at word `base` (a multiple of STEP).  VEC: the 16 bytes at
// base + 4 * tid - the plane is 16-byte aligned; else the words base + tid + 256 * k, each a load of its own (never merged: they
// are not neighbours).  FULL: the whole step lies below w1; else words at and beyond w1 count as zero and are not read.
template <bool VEC, bool FULL>
__device__ __forceinline__ u32x4 load_words(const unsigned* __restrict__ pl, int base, int tid, int w1) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if constexpr (VEC) {
    const int w = base + 4 * tid;
    if (FULL || w + 4 <= w1) v = *reinterpret_cast<const u32x4*>(pl + w);
    else {
      if (w < w1) v.x = pl[w];
      if (w + 1 < w1) v.y = pl[w + 1];
      if (w + 2 < w1) v.z = pl[w + 2];
    }
  } else {
    const int w = base + tid;
    if (FULL || w < w1) v.x = pl[w];
    if (FULL || w + OT < w1) v.y = pl[w + OT];
    if (FULL || w + 2 * OT < w1) v.z = pl[w + 2 * OT];
    if (FULL || w + 3 * OT < w1) v.w = pl[w + 3 * OT];
  }
  return v;
}
__device__ __forceinline__ int popc4(const u32x4 v, int c) {
  return c + __builtin_popcount(v.x) + __builtin_popcount(v.y) + __builtin_popcount(v.z) + __builtin_popcount(v.w);
}

template <bool VEC, bool FULL>
__device__ __forceinline__ void overlap_step(const unsigned* const (&pa)[TILE], const unsigned* const (&pb)[TILE], int base, int tid, int w1,
                                             int (&acc)[TILE * TILE], int (&ar)[2 * TILE]) {
  u32x4 A[TILE], Bv[TILE];
#pragma unroll
  for (int i = 0; i < TILE; ++i) A[i] = load_words<VEC, FULL>(pa[i], base, tid, w1);
#pragma unroll
  for (int j = 0; j < TILE; ++j) Bv[j] = load_words<VEC, FULL>(pb[j], base, tid, w1);
#pragma unroll
  for (int i = 0; i < TILE; ++i) {
    ar[i] = popc4(A[i], ar[i]);
    ar[TILE + i] = popc4(Bv[i], ar[TILE + i]);
  }
#pragma unroll
  for (int i = 0; i < TILE; ++i)
#pragma unroll
    for (int j = 0; j < TILE; ++j) acc[i * TILE + j] = popc4(A[i] & Bv[j], acc[i * TILE + j]);
}

// N per-lane values -> N / 4: afterwards v[q] of lane l is value 4 q + (l & 3) summed over the 16 lanes of l's row.  Two butterfly
// steps that halve the values (a lane keeps the value of its own bit and hands the other one to its partner), then the four quads of
// a row by two rotations (they keep l & 3).  All 64 lanes must be active; every index is a compile-time constant.
template <int N>
__device__ __forceinline__ void fold_rows(int (&v)[N], int lane) {
  const bool b0 = (lane & 1) != 0, b1 = (lane & 2) != 0;
#pragma unroll
  for (int p = 0; p < N / 2; ++p) {
    const int x = v[2 * p], y = v[2 * p + 1];
    v[p] = (b0 ? y : x) + dpp_i32<DPP_XOR1>(b0 ? x : y);
  }
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    const int x = v[2 * q], y = v[2 * q + 1];
    v[q] = (b1 ? y : x) + dpp_i32<DPP_XOR2>(b1 ? x : y);
  }
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    v[q] += dpp_i32<DPP_ROR8>(v[q]);
    v[q] += dpp_i32<DPP_ROR4>(v[q]);
  }
}

template <bool FRAMES, bool VEC>
__global__ __launch_bounds__(OT) void mask_overlap_kernel(const OverlapParams p) {
  __shared__ int red[16 * SLOT];   // one row of SLOT ints per (wave, 16-lane row)
  const la3d_overlap_tile t = p.tiles[blockIdx.x];   // (uniform)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the planes of the tile (uniform).  A row the tile does not have, or one that is refused, takes the place of another plane of the
  // tile: its counts mean nothing and the finish kernel never reads them.  No plane at all: nothing to do.
  long long oa[TILE], ob[TILE];
  const bool gok = group_ok<FRAMES>(p, t);
  const unsigned* any = nullptr;
#pragma unroll
  for (int i = TILE - 1; i >= 0; --i) {
    oa[i] = (gok && i < t.ni) ? uniform_i64(plane_at<FRAMES>(p.a_stride, p.a_off, p.a_img, p.a_words, t.row_a + i, t.g, t.nw)) : -1;
    ob[i] = (gok && i < t.nj) ? uniform_i64(plane_at<FRAMES>(p.b_stride, p.b_off, p.b_img, p.b_words, t.row_b + i, t.g, t.nw)) : -1;
    if (ob[i] >= 0) any = p.b + ob[i];
    if (oa[i] >= 0) any = p.a + oa[i];
  }
  if (!any) return;   // (uniform; before any barrier)
  const unsigned* pa[TILE];
  const unsigned* pb[TILE];
#pragma unroll
  for (int i = 0; i < TILE; ++i) {
    pa[i] = oa[i] >= 0 ? p.a + oa[i] : any;
    pb[i] = ob[i] >= 0 ? p.b + ob[i] : any;
  }
  int acc[TILE * TILE], ar[2 * TILE];
#pragma unroll
  for (int k = 0; k < TILE * TILE; ++k) acc[k] = 0;
#pragma unroll
  for (int k = 0; k < 2 * TILE; ++k) ar[k] = 0;
  const int w1 = min(t.w1, t.nw);
  int base = t.w0;                      // (a multiple of STEP)
  for (; base + STEP <= w1; base += STEP) overlap_step<VEC, true>(pa, pb, base, tid, w1, acc, ar);
  if (base < w1) overlap_step<VEC, false>(pa, pb, base, tid, w1, acc, ar);
  // 80 values of 256 lanes -> 80 ints: rows of 16 lanes by DPP, the 16 rows of the workgroup through LDS
  fold_rows<TILE * TILE>(acc, lane);
  fold_rows<2 * TILE>(ar, lane);
  if ((lane & 12) == 0) {
    int* r = red + (wave * 4 + (lane >> 4)) * SLOT + (lane & 3);
#pragma unroll
    for (int q = 0; q < TILE * TILE / 4; ++q) r[4 * q] = acc[q];
#pragma unroll
    for (int q = 0; q < 2 * TILE / 4; ++q) r[TILE * TILE + 4 * q] = ar[q];
  }
  __syncthreads();
  if (tid < SLOT) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[k * SLOT + tid];
    p.partial[(long long)blockIdx.x * SLOT + tid] = s;
  }
}

__device__ inline double overlap_ratio(int inter, int aa, int ab, int kind) {
  const int den = kind == LA3D_OVERLAP_IOU ? aa + ab - inter : kind == LA3D_OVERLAP_IOM ? min(aa, ab) : aa;
  return den == 0 ? 0.0 : (double)inter / (double)den;
}

// the chunks of a tile -> inter, areas, ratio: the workgroup of a tile's first chunk; every output element has exactly one writer
template <bool FRAMES>
__global__ __launch_bounds__(128) void mask_overlap_finish_kernel(const OverlapParams p) {
  __shared__ int sum[SLOT];
  __shared__ int okrow[2 * TILE];
  const la3d_overlap_tile t = p.tiles[blockIdx.x];   // (uniform)
  if (t.chunk != 0) return;
  const int tid = threadIdx.x;
  if (tid < SLOT) {
    const int* q = p.partial + (long long)blockIdx.x * SLOT + tid;
    int s = 0;
    for (int c = 0; c < t.nchunks; ++c) s += q[(long long)c * SLOT];
    sum[tid] = s;
  } else if (tid >= 96 && tid < 96 + 2 * TILE) {   // the decision of mask_overlap_kernel, made again
    const int k = tid - 96, i = k & 7;
    bool ok = group_ok<FRAMES>(p, t);
    if (k < TILE) ok = ok && i < t.ni && plane_at<FRAMES>(p.a_stride, p.a_off, p.a_img, p.a_words, t.row_a + i, t.g, t.nw) >= 0;
    else ok = ok && i < t.nj && plane_at<FRAMES>(p.b_stride, p.b_off, p.b_img, p.b_words, t.row_b + i, t.g, t.nw) >= 0;
    okrow[k] = ok ? 1 : 0;
  }
  __syncthreads();
  if (tid < TILE * TILE) {
    const int i = tid >> 3, j = tid & 7;
    if (i < t.ni && j < t.nj) {
      const bool ok = okrow[i] && okrow[TILE + j];
      const int v = ok ? sum[tid] : -1, aa = sum[TILE * TILE + i], ab = sum[TILE * TILE + TILE + j];
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
      const long long at = t.out0 + (long long)(t.i0 + i) * t.nb + (t.j0 + j);
      p.inter[at] = v;
      if (p.iou) p.iou[at] = ok ? overlap_ratio(v, aa, ab, p.kind) : nan;
      if (t.flags & LA3D_OVERLAP_MIRROR) {
        const long long ta = t.out0 + (long long)(t.j0 + j) * t.nb + (t.i0 + i);
        p.inter[ta] = v;
        if (p.iou) p.iou[ta] = ok ? overlap_ratio(v, ab, aa, p.kind) : nan;
      }
    }
  } else if (tid < SLOT) {
    const int k = tid - TILE * TILE, i = k & 7;
    if (k < TILE) {
      if ((t.flags & LA3D_OVERLAP_AREA_A) && i < t.ni) p.area_a[t.row_a + i] = okrow[k] ? sum[tid] : -1;
    } else {
      if ((t.flags & LA3D_OVERLAP_AREA_B) && i < t.nj && p.area_b) p.area_b[t.row_b + i] = okrow[k] ? sum[tid] : -1;
    }
  }
}

struct NmsParams {
  const int* inter; const int* area; const long long* offsets; const int* row_offsets; const int* order; const int* labels;
  double thr; int kind; unsigned char* keep;
};

// greedy NMS of one group: the rows in visiting order, one barrier per kept row; lanes over the later rows
__global__ __launch_bounds__(NMS_T) void mask_nms_kernel(const NmsParams p) {
  __shared__ unsigned char gone[NMS_MAX + 4];   // by visiting position
  const int g = blockIdx.x, tid = threadIdx.x;
  const int r0 = p.row_offsets[g], n = p.row_offsets[g + 1] - r0;   // (uniform)
  if (n <= 0) return;
  for (int k = tid; k < n; k += NMS_T) p.keep[r0 + k] = 0;
  if (n > NMS_MAX) return;
  for (int k = tid; k < n; k += NMS_T) gone[k] = 0;
  __syncthreads();
  const int* I = p.inter + p.offsets[g];
  for (int k = 0; k < n; ++k) {
    const int t = p.order[r0 + k] - r0;                       // (uniform)
    if ((unsigned)t >= (unsigned)n || gone[k]) continue;       // (uniform: gone[k] was written before the last barrier)
    const int at = p.area[r0 + t];
    if (at < 0) continue;                                      // a refused row: never kept, suppresses nothing
    if (tid == 0) p.keep[r0 + t] = 1;
    const int lt = p.labels ? p.labels[r0 + t] : 0;
    for (int q = k + 1 + tid; q < n; q += NMS_T) {
      const int u = p.order[r0 + q] - r0;
      if ((unsigned)u >= (unsigned)n || gone[q]) continue;
      if (p.labels && p.labels[r0 + u] != lt) continue;
      const int au = p.area[r0 + u];
      if (au < 0) continue;
      const int x = I[(long long)t * n + u];
      const int den = p.kind == LA3D_OVERLAP_IOM ? min(at, au) : at + au - x;
      if (den > 0 && (double)x > p.thr * (double)den) gone[q] = 1;
    }
    __syncthreads();
  }
}

inline long long tiles_of(long long n) { return (n + TILE - 1) / TILE; }

}  // namespace

extern "C" {

int64_t la3d_mask_overlap_plan(int32_t G, const int32_t* counts_a, const int32_t* counts_b, const int64_t* group_words, int64_t nwords,
                               la3d_overlap_tile* tiles, int64_t capacity, int64_t* offsets) {
  const char* who = "la3d_mask_overlap_plan";
  if (G < 0 || !offsets || (G > 0 && !counts_a) || capacity < 0 || (!group_words && nwords < 0)) return refuse(who, "G < 0, a NULL counts_a or offsets, a negative capacity or nwords");
  const bool self = counts_b == nullptr;
  long long pairs = 0, rows_a = 0, rows_b = 0, base_tiles = 0;
  for (int g = 0; g < G; ++g) {
    const long long na = counts_a[g], nb = self ? na : counts_b[g], nw = group_words ? group_words[g] : nwords;
    if (na < 0 || nb < 0 || nw < 0) return refuse(who, "a negative row count or word count");
    if (nw > MAX_WORDS) return refuse(who, "a plane of more than 2^23 words (H * W_stored > 2^28): a count would not fit int32", LA3D_ERR_UNSUPPORTED);
    pairs += na * nb; rows_a += na; rows_b += nb;
    if (pairs > MAX_PAIRS || rows_a > MAX_PAIRS || rows_b > MAX_PAIRS) return refuse(who, "more than 2^31 - 1 pairs or rows in one call", LA3D_ERR_UNSUPPORTED);
    const long long ta = tiles_of(na), tb = tiles_of(nb);
    base_tiles += self ? ta * (ta + 1) / 2 : (na == 0 ? tb : nb == 0 ? ta : ta * tb);
  }
  const long long split = base_tiles == 0 || base_tiles >= WANT_WGS ? 1 : (WANT_WGS + base_tiles - 1) / base_tiles;
  long long n = 0, out0 = 0, ra = 0, rb = 0;
  offsets[0] = 0;
  for (int g = 0; g < G; ++g) {
    const long long na = counts_a[g], nb = self ? na : counts_b[g], nw = group_words ? group_words[g] : nwords;
    const long long ta = tiles_of(na), tb = tiles_of(nb);
    long long cw = ((nw + split - 1) / split + STEP - 1) / STEP * STEP;   // words of a chunk: whole steps
    if (cw < STEP) cw = STEP;
    const long long nch = nw > 0 ? (nw + cw - 1) / cw : 1;
    // (a side without rows still has one column of tiles: they carry the other side's areas)
    for (long long ti = 0; ti < (ta ? ta : 1) && (na || nb); ++ti)
      for (long long tj = self ? ti : 0; tj < (tb ? tb : 1); ++tj)
        for (long long c = 0; c < nch; ++c, ++n) {
          if (!tiles) continue;
          if (n >= capacity) return refuse(who, "the tile table is smaller than the call needs");
          la3d_overlap_tile& t = tiles[n];
          t.g = g; t.i0 = (int)(ti * TILE); t.j0 = (int)(tj * TILE);
          t.ni = (int)(na - t.i0 < TILE ? na - t.i0 : TILE); t.nj = (int)(nb - t.j0 < TILE ? nb - t.j0 : TILE);
          t.row_a = (int)(ra + t.i0); t.row_b = (int)((self ? ra : rb) + t.j0);
          t.w0 = (int)(c * cw); t.w1 = (int)((c + 1) * cw < nw ? (c + 1) * cw : nw);
          t.nw = (int)nw; t.chunk = (int)c; t.nchunks = (int)nch; t.nb = (int)nb;
          t.flags = self ? (tj > ti ? LA3D_OVERLAP_MIRROR : LA3D_OVERLAP_AREA_A | LA3D_OVERLAP_AREA_B)
                         : (tj == 0 ? LA3D_OVERLAP_AREA_A : 0) | (ti == 0 ? LA3D_OVERLAP_AREA_B : 0);
          t.out0 = out0;
        }
    if (n > MAX_PAIRS) return refuse(who, "more than 2^31 - 1 tiles in one call", LA3D_ERR_UNSUPPORTED);
    out0 += na * nb; ra += na; rb += nb;
    offsets[g + 1] = out0;
  }
  return n;
}

size_t la3d_mask_overlap_workspace_bytes(int64_t ntiles) { return ntiles > 0 ? (size_t)ntiles * SLOT * sizeof(int) : 0; }

int la3d_mask_overlap(const la3d_mask_overlap_args* args) {
  const char* who = "la3d_mask_overlap";
  if (!args || args->struct_size != (int32_t)sizeof(la3d_mask_overlap_args)) return refuse(who, "NULL block or a struct_size that is not sizeof(la3d_mask_overlap_args)");
  const la3d_mask_overlap_args& a = *args;
  const bool self = a.b_bits == nullptr, frames = a.frames != nullptr;
  if (a.G < 0 || a.rows_a < 0 || (!self && a.rows_b < 0) || a.ntiles < 0 || a.npairs < 0) return refuse(who, "negative G, rows, ntiles or npairs");
  if (a.iou && (a.kind < LA3D_OVERLAP_IOU || a.kind > LA3D_OVERLAP_IOA)) return refuse(who, "kind must be LA3D_OVERLAP_IOU, _IOM or _IOA with iou");
  if (frames) {
    if (a.P != a.G || a.H <= 0 || a.W <= 0) return refuse(who, "frames form: G must be P (group g is image g) and the bounds H, W > 0");
    if (a.a_words < 0 || (!self && a.b_words < 0)) return refuse(who, "a_words and b_words must not be negative");
    if ((((long long)a.H * ((a.W + 31) / 32 * 32)) >> 5) > MAX_WORDS) return refuse(who, "bounds beyond H * roundup32(W) <= 2^28: a count would not fit int32", LA3D_ERR_UNSUPPORTED);
  } else {
    if (a.nwords < 0) return refuse(who, "nwords must not be negative");
    if (a.nwords > MAX_WORDS) return refuse(who, "a plane of more than 2^23 words (H * W_stored > 2^28): a count would not fit int32", LA3D_ERR_UNSUPPORTED);
  }
  if (a.npairs > MAX_PAIRS || a.ntiles > MAX_PAIRS || a.rows_a > MAX_PAIRS || (!self && a.rows_b > MAX_PAIRS))
    return refuse(who, "more than 2^31 - 1 pairs, rows or tiles in one call", LA3D_ERR_UNSUPPORTED);
  if (a.ntiles == 0) return LA3D_SUCCESS;
  // (a side without rows, or a call without pairs, has nothing to point at: a b_bits that is NULL with rows_b == 0 reads as the self
  // form, whose tiles then have no row of B either)
  if (!a.tiles || !a.workspace || (a.rows_a > 0 && (!a.a_bits || !a.area_a)) || (!self && a.rows_b > 0 && !a.area_b) || (a.npairs > 0 && !a.inter))
    return refuse(who, "NULL a_bits, tiles, inter, area_a, area_b or workspace");
  if ((at(a.a_bits) | at(a.b_bits) | at(a.inter) | at(a.area_a) | at(a.area_b) | at(a.workspace)) & 3)
    return refuse(who, "a_bits, b_bits, inter, area_a, area_b or workspace not a 4-byte aligned pointer");
  if ((at(a.tiles) | at(a.iou)) & 7) return refuse(who, "tiles or iou not an 8-byte aligned pointer");
  OverlapParams p = {};
  p.a = a.a_bits; p.b = self ? a.a_bits : a.b_bits;
  p.tiles = a.tiles; p.partial = static_cast<int*>(a.workspace);
  p.inter = a.inter; p.area_a = a.area_a; p.area_b = (self && a.area_b == a.area_a) ? nullptr : a.area_b; p.iou = a.iou; p.kind = a.kind;
  hipStream_t st = static_cast<hipStream_t>(a.stream);
  const dim3 grid((unsigned)a.ntiles);
  if (frames) {
    if (!a.a_offsets || !a.a_image_index || (!self && (!a.b_offsets || !a.b_image_index))) return refuse(who, "frames form: NULL offsets or image_index");
    if ((at(a.a_bits) | at(a.b_bits)) & 15) return refuse(who, "frames form: a_bits or b_bits not a 16-byte aligned pointer");
    if ((at(a.a_offsets) | at(a.b_offsets) | at(a.frames)) & 7) return refuse(who, "a_offsets, b_offsets or frames not an 8-byte aligned pointer");
    if ((at(a.a_image_index) | at(a.b_image_index)) & 3) return refuse(who, "a_image_index or b_image_index not a 4-byte aligned pointer");
    p.a_off = reinterpret_cast<const long long*>(a.a_offsets); p.a_img = a.a_image_index; p.a_words = a.a_words;
    p.b_off = self ? p.a_off : reinterpret_cast<const long long*>(a.b_offsets);
    p.b_img = self ? p.a_img : a.b_image_index; p.b_words = self ? a.a_words : a.b_words;
    p.frames = a.frames; p.P = a.P; p.H = a.H; p.W = a.W;
    hipLaunchKernelGGL((mask_overlap_kernel<true, true>), grid, dim3(OT), 0, st, p);
    const int rc = check_launch("mask_overlap_kernel");
    if (rc != LA3D_SUCCESS) return rc;
    hipLaunchKernelGGL(mask_overlap_finish_kernel<true>, grid, dim3(128), 0, st, p);
    return check_launch("mask_overlap_finish_kernel");
  }
  if (a.a_stride < a.nwords || (!self && a.b_stride < a.nwords)) return refuse(who, "a_stride or b_stride below nwords");
  p.a_stride = a.a_stride; p.b_stride = self ? a.a_stride : a.b_stride;
  const bool vec = ((at(p.a) | at(p.b)) & 15) == 0 && (p.a_stride & 3) == 0 && (p.b_stride & 3) == 0;
  if (vec) hipLaunchKernelGGL((mask_overlap_kernel<false, true>), grid, dim3(OT), 0, st, p);
  else hipLaunchKernelGGL((mask_overlap_kernel<false, false>), grid, dim3(OT), 0, st, p);
  const int rc = check_launch("mask_overlap_kernel");
  if (rc != LA3D_SUCCESS) return rc;
  hipLaunchKernelGGL(mask_overlap_finish_kernel<false>, grid, dim3(128), 0, st, p);
  return check_launch("mask_overlap_finish_kernel");
}

int la3d_mask_nms(const la3d_mask_nms_args* args) {
  const char* who = "la3d_mask_nms";
  if (!args || args->struct_size != (int32_t)sizeof(la3d_mask_nms_args)) return refuse(who, "NULL block or a struct_size that is not sizeof(la3d_mask_nms_args)");
  const la3d_mask_nms_args& a = *args;
  if (a.G < 0 || a.B < 0) return refuse(who, "negative G or B");
  if (a.kind != LA3D_OVERLAP_IOU && a.kind != LA3D_OVERLAP_IOM) return refuse(who, "kind must be LA3D_OVERLAP_IOU or LA3D_OVERLAP_IOM");
  if (!(a.thr == a.thr)) return refuse(who, "thr must not be NaN");
  if (a.B > MAX_PAIRS) return refuse(who, "more than 2^31 - 1 rows in one call", LA3D_ERR_UNSUPPORTED);
  if (a.G == 0 || a.B == 0) return LA3D_SUCCESS;
  if (!a.inter || !a.area || !a.offsets || !a.row_offsets || !a.order || !a.keep) return refuse(who, "NULL inter, area, offsets, row_offsets, order or keep");
  if ((at(a.inter) | at(a.area) | at(a.row_offsets) | at(a.order) | at(a.labels)) & 3) return refuse(who, "inter, area, row_offsets, order or labels not a 4-byte aligned pointer");
  if (at(a.offsets) & 7) return refuse(who, "offsets not an 8-byte aligned pointer");
  NmsParams p = {a.inter, a.area, reinterpret_cast<const long long*>(a.offsets), a.row_offsets, a.order, a.labels, a.thr, a.kind, a.keep};
  hipLaunchKernelGGL(mask_nms_kernel, dim3((unsigned)a.G), dim3(NMS_T), 0, static_cast<hipStream_t>(a.stream), p);
  return check_launch("mask_nms_kernel");
}

}  // extern "C"
