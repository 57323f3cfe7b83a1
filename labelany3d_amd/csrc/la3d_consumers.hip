// la3d_consumers.hip - the steps around the path: box consumers (src/tools/combine_results.py:105-124, :238-252), the masked
// depth-ratio median and the depth-alignment selection / scatter (src/util.py:464-494, src/batch_scripts/depth.py:52-92), the matcher's
// unprojection (src/matching/matcher.py:70-91).  Split out of la3d_aux.hip in round 6.
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
#include "la3d_select.hpp"

using namespace la3d;

namespace {
// Box consumers (reference src/tools/combine_results.py:105-108, :238-252): project the 8 corners of every
// record with its image's K, 2-D AABB and its clamp to the frame.  One thread per box.
__global__ __launch_bounds__(128) void project_boxes_kernel(const double* __restrict__ rec, const double* __restrict__ K,
                                                            int k_stride, const int* __restrict__ image_index, int B,
                                                            double Wd, double Hd, double* __restrict__ out) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= B) return;
  const double* k = K + (long long)(image_index ? image_index[i] : i) * k_stride;
  const double* c = rec + (long long)i * LA3D_REC + 15;
  double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
  bool bad = false;
  for (int v = 0; v < 8; ++v) {
    double px, py;
    project_corner(k, c[v * 3], c[v * 3 + 1], c[v * 3 + 2], &px, &py);   // (K @ P)[:2] / (K @ P)[2]
    if (px != px || py != py) bad = true;              // Python's min()/max() over NaN are order dependent: report NaN
    lo[0] = fmin(lo[0], px); hi[0] = fmax(hi[0], px);
    lo[1] = fmin(lo[1], py); hi[1] = fmax(hi[1], py);
  }
  double* o = out + (long long)i * 8;
  if (bad) { for (int j = 0; j < 8; ++j) o[j] = NAN; return; }
  o[0] = lo[0]; o[1] = lo[1]; o[2] = hi[0]; o[3] = hi[1];
  o[4] = fmax(0.0, lo[0]); o[5] = fmax(0.0, lo[1]); o[6] = fmin(Wd, hi[0]); o[7] = fmin(Hd, hi[1]);
}

// IoU of every pair of xyxy boxes (iou2D, reference src/tools/combine_results.py:111-124): the negated matrix is
// the Hungarian cost matrix of :131-135.
__device__ __forceinline__ double iou2d(const double* __restrict__ p, const double* __restrict__ q) {
  const double x1 = fmax(p[0], q[0]), y1 = fmax(p[1], q[1]), x2 = fmin(p[2], q[2]), y2 = fmin(p[3], q[3]);
  const double inter = fmax(0.0, x2 - x1) * fmax(0.0, y2 - y1);
  return inter / ((p[2] - p[0]) * (p[3] - p[1]) + (q[2] - q[0]) * (q[3] - q[1]) - inter + 1e-6);
}
__global__ __launch_bounds__(256) void iou_matrix_kernel(const double* __restrict__ a, int na, const double* __restrict__ b,
                                                         int nb, double* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)na * nb) return;
  out[t] = iou2d(a + (t / nb) * 4, b + (t % nb) * 4);
}

// The same for G groups in one launch (la3d_iou_matrix_groups): element t of [0, npairs) finds its group in offsets - the last g with
// offsets[g] <= t - and its pair in the group's row-major matrix.  Every table value is checked before a box is addressed with it: an
// element that lies in no group's matrix, or whose rows lie outside the boxes, gets NaN.
struct IouGroupsParams {
  const double* a; const double* b; long long rows_a, rows_b;
  const int* row_a; const int* row_b; const long long* offsets; long long npairs; double* out; int G;
};
__global__ __launch_bounds__(256) void iou_matrix_groups_kernel(const IouGroupsParams p) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= p.npairs) return;
  int lo = 0, hi = p.G - 1;          // (G >= 1)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.offsets[mid] <= t) lo = mid; else hi = mid - 1;
  }
  const long long k = t - p.offsets[lo];
  const long long a0 = p.row_a[lo], na = (long long)p.row_a[lo + 1] - a0, b0 = p.row_b[lo], nb = (long long)p.row_b[lo + 1] - b0;
  double r = NAN;
  if (k >= 0 && na > 0 && nb > 0 && k < na * nb && a0 >= 0 && a0 + na <= p.rows_a && b0 >= 0 && b0 + nb <= p.rows_b)
    r = iou2d(p.a + (a0 + k / nb) * 4, p.b + (b0 + k % nb) * 4);
  p.out[t] = r;
}

// Masked depth-ratio median — reference src/util.py:476-486 (align_to_depth_match): overlap = mask_a & mask_b,
// scale = np.median(num[overlap] / den[overlap]) in float32.  One 512-thread workgroup per instance:
//   phase 1  the two u8 masks are read once with 16-byte loads into an overlap bit image in LDS;
//   median   the exact selection of la3d_select.hpp (masked_median: sample -> bracket -> collect -> select in LDS, with the four radix
//            rounds behind it; round 3: 650 -> 360 us per 1024 VGA instances, identical results) over the ratio of the two planes.
// Any NaN ratio makes the result NaN, as np.median does; an empty overlap gives count 0, NaN.
struct RatioValue {          // the VALUE of la3d_select.hpp: num / den, both loaded before the division
  const float* num; const float* den;
  struct In { float a, d; };
  __device__ In idle() const { return {0.f, 1.f}; }
  __device__ In load(int i) const { return {num[i], den[i]}; }
  __device__ float value(const In& x) const { return x.a / x.d; }
};

__global__ __launch_bounds__(RM_NT) void ratio_median_kernel(const float* __restrict__ num, long long num_stride,
                                                           const int* __restrict__ image_index, const float* __restrict__ den,
                                                           const unsigned char* __restrict__ mask_a,
                                                           const unsigned char* __restrict__ mask_b, int HW, int nwords,
                                                           float* __restrict__ median, int* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  unsigned* hist = bits + ((nwords + 3) & ~3);   // fallback rounds: [256][RM_COPIES]; fast path: the key buffer, RM_CAP words
  static_assert(RM_CAP >= 256 * RM_COPIES, "the key buffer also holds the fallback's histogram");
  unsigned* h1 = hist + RM_CAP;                  // fast path: [256][4] bins of the bracket; lds_select2: [2][256]
  unsigned* bsum = h1 + 1024;                    // [256] bin totals
  unsigned* misc = bsum + 256;                   // [0] n, [6] number of active chunks; then masked_median's (it leaves [6] alone)
  unsigned short* clist = reinterpret_cast<unsigned short*>(misc + 16);   // ids of the 64-pixel chunks holding an overlap pixel
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, inst = blockIdx.x;
  const float* np_ = num + (long long)(image_index ? image_index[inst] : inst) * num_stride;
  const float* dp = den + (long long)inst * HW;
  const unsigned char* ma = mask_a + (long long)inst * HW;
  const unsigned char* mb = mask_b ? mask_b + (long long)inst * HW : nullptr;
  if (tid < 16) misc[tid] = tid == 5 ? 0xffffffffu : 0u;
  // ---- phase 1: overlap bit image ----
  unsigned n_local = 0;
  const bool vec = (HW % 16 == 0) && ((reinterpret_cast<uintptr_t>(ma) & 15) == 0) && (!mb || (reinterpret_cast<uintptr_t>(mb) & 15) == 0);
  if (vec) {
    unsigned short* b16 = reinterpret_cast<unsigned short*>(bits);
    const u32x4* a4 = reinterpret_cast<const u32x4*>(ma);
    const u32x4* b4 = reinterpret_cast<const u32x4*>(mb);
    const int ngroups = HW >> 4;
#pragma unroll 4
    for (int g = tid; g < ngroups; g += RM_NT) {
      const u32x4 wa = __builtin_nontemporal_load(a4 + g);
      unsigned pat = nz16(wa.x, wa.y, wa.z, wa.w);
      if (mb) {
        const u32x4 wb = __builtin_nontemporal_load(b4 + g);
        pat &= nz16(wb.x, wb.y, wb.z, wb.w);
      }
      b16[g] = (unsigned short)pat;
      n_local += __popc(pat);
    }
    if ((ngroups & 1) && tid == 0) b16[ngroups] = 0;
  } else {
    for (int w = tid; w < nwords; w += RM_NT) {
      unsigned word = 0;
      const int i0 = w * 32;
      for (int k = 0; k < 32; ++k) {
        const int i = i0 + k;
        if (i < HW && ma[i] && (!mb || mb[i])) word |= 1u << k;
      }
      bits[w] = word;
      n_local += __popc(word);
    }
  }
  n_local = (unsigned)wave_sum_i((int)n_local);
  __syncthreads();                       // misc is initialised
  if (lane == 0) atomicAdd(&misc[0], n_local);
  __syncthreads();
  const unsigned n = misc[0];
  if (n == 0) {
    if (tid == 0) { median[inst] = NAN; count[inst] = 0; }
    return;
  }
  list_active_chunks(bits, nwords, (HW + 63) >> 6, clist, &misc[6], tid);   // the median visits only chunks with an overlap pixel
  __syncthreads();
  const float med = masked_median(RatioValue{np_, dp}, n, bits, nwords, clist, (int)misc[6], hist, h1, bsum, misc, tid);
  if (tid == 0) { median[inst] = med; count[inst] = (int)n; }
}

// ---- align_depth support (reference src/batch_scripts/depth.py:52-92) -----------------------------------------------
// valid = ~isinf(relative) & (metric < max_valid) [& mask]; the regressor (scikit-learn RANSAC, third party, random) is fed
// relative[valid], metric[valid] in row-major order, and its prediction is scattered back over a 10000.0-filled frame.
// Order-preserving stream compaction in three small kernels: per-tile counts, scan of the counts, scatter.
constexpr int AL_TILE = 4096;   // elements per 256-thread workgroup (16 per thread, four float4)

__device__ inline bool align_valid(float rel, float met, unsigned char m, bool has_mask, float max_valid) {
  const bool isinf_rel = (__float_as_uint(rel) & 0x7fffffffu) == 0x7f800000u;   // np.isinf: NaN is NOT excluded
  return !isinf_rel && (met < max_valid) && (!has_mask || m != 0);
}

__global__ __launch_bounds__(256) void align_count_kernel(const float* __restrict__ rel, const float* __restrict__ met,
                                                          const unsigned char* __restrict__ mask, long long n, float max_valid,
                                                          long long* __restrict__ counts) {
  __shared__ int part[4];
  // blockIdx.y = frame of a batch (la3d_align_select_batch): planes n apart, (gridDim.x + 1) count slots per frame
  rel += (long long)blockIdx.y * n; met += (long long)blockIdx.y * n;
  if (mask) mask += (long long)blockIdx.y * n;
  counts += (long long)blockIdx.y * (gridDim.x + 1);
  const long long base = (long long)blockIdx.x * AL_TILE;
  int c = 0;
  for (int k = 0; k < AL_TILE / 256; ++k) {
    const long long i = base + k * 256 + threadIdx.x;
    if (i < n) c += align_valid(rel[i], met[i], mask ? mask[i] : 1, mask != nullptr, max_valid) ? 1 : 0;
  }
  c = wave_sum_i(c);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// exclusive scan of the tile counts in place, total appended at counts[nb]; one workgroup
__global__ __launch_bounds__(256) void align_scan_kernel(long long* __restrict__ counts, int nb, long long* __restrict__ total) {
  __shared__ long long carry;
  __shared__ long long wsum[4];
  counts += (long long)blockIdx.x * (nb + 1);   // one workgroup per frame
  total += blockIdx.x;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nb; b0 += 256) {
    const int b = b0 + threadIdx.x;
    const long long v = b < nb ? counts[b] : 0;
    long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long t = __shfl_up(incl, o);
      if ((threadIdx.x & 63) >= o) incl += t;
    }
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    long long off = carry;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) off += wsum[w];
    if (b < nb) counts[b] = off + incl - v;
    __syncthreads();
    if (threadIdx.x == 255) carry = off + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) { counts[nb] = carry; *total = carry; }
}

__global__ __launch_bounds__(256) void align_scatter_kernel(const float* __restrict__ rel, const float* __restrict__ met,
                                                            const unsigned char* __restrict__ mask, long long n, float max_valid,
                                                            const long long* __restrict__ offsets, float* __restrict__ rel_out,
                                                            float* __restrict__ met_out) {
  __shared__ int wtot[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  rel += (long long)blockIdx.y * n; met += (long long)blockIdx.y * n;       // frame of a batch: outputs have capacity n per frame
  if (mask) mask += (long long)blockIdx.y * n;
  rel_out += (long long)blockIdx.y * n; met_out += (long long)blockIdx.y * n;
  offsets += (long long)blockIdx.y * (gridDim.x + 1);
  const long long base = (long long)blockIdx.x * AL_TILE;
  long long out = offsets[blockIdx.x];
  for (int k = 0; k < AL_TILE / 256; ++k) {   // 256 consecutive elements per step: row-major order is kept
    const long long i = base + k * 256 + threadIdx.x;
    float r = 0.f, m = 0.f;
    bool v = false;
    if (i < n) { r = rel[i]; m = met[i]; v = align_valid(r, m, mask ? mask[i] : 1, mask != nullptr, max_valid); }
    const unsigned long long bal = __ballot(v);
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    long long pos = out;
    for (int w = 0; w < wave; ++w) pos += wtot[w];
    const int step_total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    if (v) {
      pos += __popcll(bal & ((1ull << lane) - 1ull));
      rel_out[pos] = r;
      met_out[pos] = m;
    }
    out += step_total;
    __syncthreads();
  }
}

// depth = full(fill); depth[sel] = relative[sel] * coef + intercept, sel = mask (if given) else ~isinf(relative)  (:82-90)
__global__ __launch_bounds__(256) void align_apply_kernel(const float* __restrict__ rel, const unsigned char* __restrict__ mask,
                                                          long long n, float coef, float intercept, float fill,
                                                          float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float r = rel[i];
  const bool sel = mask ? mask[i] != 0 : (__float_as_uint(r) & 0x7fffffffu) != 0x7f800000u;
  // LinearRegression.predict on float32: X @ coef_.T (one float32 product, rounded) + intercept_ (rounded again).  The two roundings
  // must survive the compiler: `__fadd_rn(__fmul_rn(..))` are plain operations for hipcc and were contracted into one fma - a last-bit
  // difference for a non-zero intercept (the reference fits without one, depth.py:66, so its own calls never saw it; found by
  // profiles/r06/fuzz_aux.py, round 6)
  float y;
  {
#pragma clang fp contract(off)
    const float prod = r * coef;
    y = prod + intercept;
  }
  out[i] = sel ? y : fill;
}

// Sparse unprojection at match points — reference src/matching/matcher.py:70-91: depth looked up at
// (int(v), int(u)), points with depth == -1 dropped, u' = flip - u, v' = flip - v (flip = 512 there),
// p = ((u'-cx) d / fx, (v'-cy) d / fy, d), world = R (p - T).  One thread per match.
struct MatchParams {
  double fx, fy, cx, cy, flip;
  double R[9], T[3];
  int has_rt, use_flip;
  int H, W, N;
};
__global__ __launch_bounds__(128) void unproject_matches_kernel(const float* __restrict__ depth, const double* __restrict__ uv,
                                                                const MatchParams p, double* __restrict__ out,
                                                                int* __restrict__ valid) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= p.N) return;
  const double mu = uv[2 * i], mv = uv[2 * i + 1];
  const long long cu = (long long)mu, cv = (long long)mv;    // astype(int): truncation toward zero
  double* o = out + (long long)i * 3;
  bool ok = cu >= 0 && cu < p.W && cv >= 0 && cv < p.H;
  float df = -1.f;
  if (ok) df = depth[cv * p.W + cu];
  ok = ok && (df != -1.f);
  valid[i] = ok ? 1 : 0;
  if (!ok) { o[0] = o[1] = o[2] = NAN; return; }
  const double d = (double)df;
  const double u = p.use_flip ? p.flip - mu : mu, v = p.use_flip ? p.flip - mv : mv;
  double q[3] = {(u - p.cx) * d / p.fx, (v - p.cy) * d / p.fy, d};
  if (p.has_rt) {
    const double a = q[0] - p.T[0], b = q[1] - p.T[1], c = q[2] - p.T[2];
    q[0] = p.R[0] * a + p.R[1] * b + p.R[2] * c;
    q[1] = p.R[3] * a + p.R[4] * b + p.R[5] * c;
    q[2] = p.R[6] * a + p.R[7] * b + p.R[8] * c;
  }
  o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
}

}  // namespace

// ==========================================================================================
// C-ABI
// ==========================================================================================
extern "C" {

int la3d_masked_ratio_median(const float* num, int64_t num_plane_stride, const int32_t* image_index, const float* den,
                             const uint8_t* mask_a, const uint8_t* mask_b, int B, int H, int W, float* median,
                             int32_t* count, void* stream) {
  if (!num || !den || !mask_a || !median || !count || B < 0 || H <= 0 || W <= 0 || num_plane_stride < 0)
    return refuse("la3d_masked_ratio_median", "bad argument (null pointer, negative size or stride)");
  if (B == 0) return LA3D_SUCCESS;
  // ONE size limit, from the LDS the kernel needs: bit image + chunk list + key buffer in one CU's 160 KiB (about 819 k pixels)
  const long long HWl = (long long)H * W;
  const long long nwl = (HWl + 31) / 32;
  const long long ldsl = ((nwl + 3) & ~3LL) * 4 + (long long)(RM_CAP + 1024 + 256 + 16) * 4 + ((HWl + 63) / 64) * 2 + 16;
  if (ldsl > 160 * 1024)
    return refuse("la3d_masked_ratio_median", "frame too large for the LDS bit image (H*W up to about 819200)", LA3D_ERR_UNSUPPORTED);
  const int HW = (int)HWl, nwords = (int)nwl;
  const size_t lds = (size_t)ldsl;
  allow_big_lds(reinterpret_cast<const void*>(ratio_median_kernel));
  hipLaunchKernelGGL(ratio_median_kernel, dim3(B), dim3(RM_NT), lds, static_cast<hipStream_t>(stream), num,
                     (long long)num_plane_stride, image_index, den, mask_a, mask_b, HW, nwords, median, count);
  return check_launch("ratio_median_kernel");
}

size_t la3d_align_workspace_bytes(int64_t n) {
  if (n <= 0) return 8;
  return (size_t)((n + AL_TILE - 1) / AL_TILE + 2) * 8;   // per frame: la3d_align_select_batch needs P times this
}

int la3d_align_select_batch(const float* relative, const float* metric, const uint8_t* mask, int P, int64_t n,
                            float max_valid_depth, float* relative_out, float* metric_out, int64_t* counts, void* workspace,
                            void* stream) {
  if (P < 0 || P > 65535 || n < 0 || (P > 0 && (!counts || !workspace)) ||
      (P > 0 && n > 0 && (!relative || !metric || !relative_out || !metric_out)))
    return refuse("la3d_align_select_batch", "bad argument (P <= 65535)");
  if (P == 0) return LA3D_SUCCESS;
  hipStream_t s = static_cast<hipStream_t>(stream);
  long long* tile_counts = static_cast<long long*>(workspace);   // [P][nb + 1]
  const int nb = (int)((n + AL_TILE - 1) / AL_TILE);
  if (nb > 0)
    hipLaunchKernelGGL(align_count_kernel, dim3(nb, P), dim3(256), 0, s, relative, metric, mask, (long long)n, max_valid_depth,
                       tile_counts);
  hipLaunchKernelGGL(align_scan_kernel, dim3(P), dim3(256), 0, s, tile_counts, nb, reinterpret_cast<long long*>(counts));
  if (nb > 0)
    hipLaunchKernelGGL(align_scatter_kernel, dim3(nb, P), dim3(256), 0, s, relative, metric, mask, (long long)n, max_valid_depth,
                       tile_counts, relative_out, metric_out);
  return check_launch("align_select_batch");
}

int la3d_align_select(const float* relative, const float* metric, const uint8_t* mask, int64_t n, float max_valid_depth,
                      float* relative_out, float* metric_out, int64_t* count, void* workspace, void* stream) {
  if (n < 0 || !count || !workspace || (n > 0 && (!relative || !metric || !relative_out || !metric_out)))
    return refuse("la3d_align_select", "bad argument");
  return la3d_align_select_batch(relative, metric, mask, 1, n, max_valid_depth, relative_out, metric_out, count, workspace, stream);
}

int la3d_align_apply(const float* relative, const uint8_t* mask, int64_t n, float coef, float intercept, float fill,
                     float* out, void* stream) {
  if (n < 0 || (n > 0 && (!relative || !out))) return refuse("la3d_align_apply", "bad argument");
  if (n == 0) return LA3D_SUCCESS;
  hipLaunchKernelGGL(align_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     relative, mask, (long long)n, coef, intercept, fill, out);
  return check_launch("align_apply_kernel");
}

int la3d_unproject_matches(const float* depth, int H, int W, const double* uv, int N, double fx, double fy, double cx,
                           double cy, int use_flip, double flip, const double* R9, const double* T3, double* out,
                           int32_t* valid, void* stream) {
  if (!depth || (!uv && N > 0) || !out || !valid || N < 0 || H <= 0 || W <= 0 || (R9 == nullptr) != (T3 == nullptr))
    return refuse("la3d_unproject_matches", "bad argument");
  if (N == 0) return LA3D_SUCCESS;
  MatchParams p;
  p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy; p.flip = flip; p.use_flip = use_flip; p.H = H; p.W = W; p.N = N;
  p.has_rt = R9 != nullptr;
  for (int i = 0; i < 9; ++i) p.R[i] = R9 ? R9[i] : 0.0;
  for (int i = 0; i < 3; ++i) p.T[i] = T3 ? T3[i] : 0.0;
  hipLaunchKernelGGL(unproject_matches_kernel, dim3((N + 127) / 128), dim3(128), 0, static_cast<hipStream_t>(stream), depth, uv,
                     p, out, valid);
  return check_launch("unproject_matches_kernel");
}

int la3d_project_boxes(const double* records, const double* K, int32_t k_stride, const int32_t* image_index, int B,
                       double width, double height, double* out, void* stream) {
  if ((!records && B > 0) || !K || !out || B < 0 || (k_stride != 0 && k_stride < 9)) return refuse("la3d_project_boxes", "bad argument");
  if (B == 0) return LA3D_SUCCESS;
  hipLaunchKernelGGL(project_boxes_kernel, dim3((B + 127) / 128), dim3(128), 0, static_cast<hipStream_t>(stream), records, K,
                     k_stride, image_index, B, width, height, out);
  return check_launch("project_boxes_kernel");
}

int la3d_iou_matrix(const double* boxes_a, int na, const double* boxes_b, int nb, double* out, void* stream) {
  if (na < 0 || nb < 0 || ((!boxes_a || !boxes_b || !out) && na > 0 && nb > 0)) return refuse("la3d_iou_matrix", "bad argument");
  if (na == 0 || nb == 0) return LA3D_SUCCESS;
  const long long n = (long long)na * nb;
  hipLaunchKernelGGL(iou_matrix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     boxes_a, na, boxes_b, nb, out);
  return check_launch("iou_matrix_kernel");
}

int la3d_iou_matrix_groups(const la3d_iou_groups_args* args) {
  const char* who = "la3d_iou_matrix_groups";
  if (!args || args->struct_size != (int32_t)sizeof(la3d_iou_groups_args)) return refuse(who, "NULL block or a struct_size that is not sizeof(la3d_iou_groups_args)");
  const la3d_iou_groups_args& a = *args;
  if (a.G < 0 || a.rows_a < 0 || a.rows_b < 0 || a.npairs < 0) return refuse(who, "negative G, rows_a, rows_b or npairs");
  if (a.G == 0 || a.npairs == 0) return LA3D_SUCCESS;
  if (a.npairs > 0x7fffffffLL * 256) return refuse(who, "more than 2^39 pairs in one call", LA3D_ERR_UNSUPPORTED);
  if (!a.boxes_a || !a.boxes_b || !a.row_offsets_a || !a.row_offsets_b || !a.offsets || !a.out) return refuse(who, "NULL boxes_a, boxes_b, row_offsets_a, row_offsets_b, offsets or out");
  const auto at = [](const void* q) { return reinterpret_cast<uintptr_t>(q); };
  if ((at(a.boxes_a) | at(a.boxes_b) | at(a.offsets) | at(a.out)) & 7) return refuse(who, "boxes_a, boxes_b, offsets or out not an 8-byte aligned pointer");
  if ((at(a.row_offsets_a) | at(a.row_offsets_b)) & 3) return refuse(who, "row_offsets_a or row_offsets_b not a 4-byte aligned pointer");
  const IouGroupsParams p = {a.boxes_a, a.boxes_b, a.rows_a, a.rows_b, a.row_offsets_a, a.row_offsets_b,
                             reinterpret_cast<const long long*>(a.offsets), a.npairs, a.out, a.G};
  hipLaunchKernelGGL(iou_matrix_groups_kernel, dim3((unsigned)((a.npairs + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(a.stream), p);
  return check_launch("iou_matrix_groups_kernel");
}

}  // extern "C"
