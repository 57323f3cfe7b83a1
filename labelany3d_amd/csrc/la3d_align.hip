// la3d_align.hip - the estimator of align_depth on the device (reference src/batch_scripts/depth.py:52-92): scikit-learn's
// RANSACRegressor(LinearRegression(fit_intercept=False), min_samples=...) for P frames in one call, between la3d_align_select_batch and
// the prediction scatter.  The model is y = a x with a median-based threshold; every quantity is a sum, a count or an exact order
// statistic.  Semantics: include/la3d.h "depth alignment: RANSAC scale fit" (restated in tests/align_ransac_cases.py).
//
// One call is a linear chain of six launches on the caller's stream, without host synchronisation, allocation or read-back:
//   threshold   one workgroup per frame: non-finite check, m, thr = median(|y - median(y)|) by two exact radix selects
//   subsets     one workgroup per (trial, frame): sum xy, sum xx of the trial's subset (fp64, fixed order) -> slope a_t
//   candidates  one workgroup per 4096 samples: ONE sweep judges all T slopes; per trial k, sum y, sum y^2, sum r^2, min / max y
//   scan        one workgroup per frame: merges the segment rows in fixed order, scores, walks the trials under scikit-learn's rule
//   refit       one workgroup per 4096 samples: sum xy, sum xx over the inliers of the best slope
//   finish      one wave per frame: coef
// No floating-point atomics anywhere: every merge has a fixed order, so a call is reproducible run to run and a frame's result does
// not depend on the batch it is in.
#include <cstddef>
#include <cstdint>

#include "la3d_device.hpp"
#include "la3d_draw.hpp"

using namespace la3d;

namespace {

constexpr int AR_NT = 256;               // threads of the sample-parallel kernels
constexpr int AR_PER = 16;               // samples per thread
constexpr int AR_SEG = AR_NT * AR_PER;   // samples per workgroup (4096)
constexpr int AR_ROWS = AR_NT / 64;      // waves per workgroup
constexpr int TH_NT = 1024;              // threads of the threshold kernel
constexpr int TH_U = 8;                 // loads a thread of the threshold kernel keeps in flight
constexpr int TH_COPIES = 16;            // copies per histogram bin (depths share their leading bits: see la3d_consumers.hip)
constexpr int FLAG_NONFINITE = 1, FLAG_BAD_INDEX = 2, FLAG_BAD_SIZE = 4;

// per-frame header in the workspace
struct ArHdr {
  float thr, ymed;
  int flags, m;
  float a_best;
  int pad[3];
};

// the workspace of a call (all offsets 16-byte aligned)
struct ArLayout {
  long long nseg, rows;
  size_t hdr, slopes, xy, pk, pmn, pmx, psy, psyy, psrr, rf, total;
};
inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
inline ArLayout ar_layout(long long P, long long n, long long T) {
  ArLayout L;
  L.nseg = n > 0 ? (n + AR_SEG - 1) / AR_SEG : 1;
  L.rows = L.nseg;
  const size_t cell = (size_t)P * (size_t)L.rows * (size_t)T;
  size_t o = 0;
  L.hdr = o; o = up16(o + (size_t)P * sizeof(ArHdr));
  L.slopes = o; o = up16(o + (size_t)P * T * 4);
  L.xy = o; o = up16(o + (size_t)P * (size_t)(n > 0 ? n : 0) * 8);
  L.pk = o; o = up16(o + cell * 4);
  L.pmn = o; o = up16(o + cell * 4);
  L.pmx = o; o = up16(o + cell * 4);
  L.psy = o; o = up16(o + cell * 8);
  L.psyy = o; o = up16(o + cell * 8);
  L.psrr = o; o = up16(o + cell * 8);
  L.rf = o; o = up16(o + (size_t)P * L.nseg * 16);
  L.total = o;
  return L;
}

struct ArParams {
  const float* x;
  const float* y;
  const long long* counts;
  long long stride;          // samples between frames (the capacity n of a row)
  double min_samples, stop_probability;
  int T, m_cap;
  const int* subsets;
  unsigned long long seed;
  float* coef;
  int *n_inliers, *n_trials, *best_trial, *status;
  ArHdr* hdr;
  float* slopes;
  float2* xy;                // [P][stride] the samples interleaved (x, y): one 8-byte gather per subset entry
  int* pk;
  float *pmn, *pmx;
  double *psy, *psyy, *psrr, *rf;
  long long nseg, rows;
};

// order-preserving key of a float32 (la3d_consumers.hip: f32_key)
__device__ inline unsigned ar_key(float v) {
  const unsigned b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ inline float ar_unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// samples of frame p: its count when it fits the row, -1 otherwise (a failed fit, before anything is addressed by it)
__device__ inline long long ar_count(const ArParams& q, int p) {
  const long long c = q.counts[p];
  return (c < 0 || c > q.stride) ? -1 : c;
}

// m of a frame with n samples: ceil(min_samples * n) in float64 below 1, min_samples itself from 1 on (the host refuses a fraction there)
__device__ inline long long ar_subset_size(double min_samples, long long n) {
  if (min_samples < 1.0) return (long long)ceil(min_samples * (double)n);
  return (long long)min_samples;
}

// ---- the device draw: la3d_draw.hpp (ar_subset_index), shared with the plane fit ---------------------------------------------------

// ---- threshold ------------------------------------------------------------------------------------------------------------------
// Keys of the values at 0-based ranks (n-1)/2 and n/2 among key(y[i]) (MODE 0) or key(|y[i] - med|) (MODE 1), i < n: most-significant-
// first radix select, four rounds of 8 bits over the samples in memory (they sit in L2), 16 copies per bin.  The upper middle key of an
// even count equals the lower one when that key occurs often enough behind the rank, otherwise it is the smallest key above it
// (one more sweep).  Every thread of the workgroup calls it; uniform results.
template <int MODE>
__device__ inline unsigned th_key(float y, float med) {
  return MODE == 0 ? ar_key(y) : ar_key(fabsf(y - med));
}
template <int MODE>
__device__ inline void th_select(const float* __restrict__ y, int n, float med, unsigned* hist, unsigned* st, int tid, unsigned* klo,
                                 unsigned* khi) {
  const int lane = tid & 63, copy = tid & (TH_COPIES - 1);
  unsigned prefix = 0, pmask = 0, rank = (unsigned)(n - 1) / 2u, cnt = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < 256 * TH_COPIES; i += TH_NT) hist[i] = 0u;
    __syncthreads();
    for (int i0 = tid; i0 < n; i0 += TH_NT * TH_U) {   // TH_U loads in flight per thread, then their histogram updates
      float v[TH_U];
#pragma unroll
      for (int u = 0; u < TH_U; ++u) { const int i = i0 + u * TH_NT; v[u] = y[i < n ? i : i0]; }
#pragma unroll
      for (int u = 0; u < TH_U; ++u) {
        const unsigned k = th_key<MODE>(v[u], med);
        if (i0 + u * TH_NT < n && (k & pmask) == prefix) atomicAdd(&hist[((k >> shift) & 0xffu) * TH_COPIES + copy], 1u);
      }
    }
    __syncthreads();
    if (tid < 64) {                      // four bins per lane, exclusive scan over the lanes
      unsigned b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned s = 0;
#pragma unroll
        for (int c = 0; c < TH_COPIES; ++c) s += hist[(4 * lane + j) * TH_COPIES + c];
        b[j] = s;
      }
      const unsigned mine = b[0] + b[1] + b[2] + b[3];
      unsigned incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
      }
      const unsigned excl = incl - mine;
      if (excl <= rank && rank < incl) { // exactly one lane
        unsigned acc = excl, bsel = 0, bc = b[0];
        if (rank >= acc + b[0]) { acc += b[0]; bsel = 1; bc = b[1];
          if (rank >= acc + b[1]) { acc += b[1]; bsel = 2; bc = b[2];
            if (rank >= acc + b[2]) { acc += b[2]; bsel = 3; bc = b[3]; } } }
        st[0] = prefix | ((4u * (unsigned)lane + bsel) << shift);
        st[1] = rank - acc;
        st[2] = bc;
      }
    }
    __syncthreads();
    prefix = st[0]; rank = st[1]; cnt = st[2];
    pmask |= 0xffu << shift;
    __syncthreads();
  }
  *klo = prefix;
  *khi = prefix;
  if ((n & 1) == 0 && rank + 1u >= cnt) {   // uniform: the upper middle value is the smallest key above the lower one
    if (tid == 0) st[3] = 0xffffffffu;
    __syncthreads();
    unsigned best = 0xffffffffu;
#pragma unroll TH_U
    for (int i = tid; i < n; i += TH_NT) {
      const unsigned k = th_key<MODE>(y[i], med);
      if (k > prefix) best = min(best, k);
    }
    atomicMin(&st[3], best);
    __syncthreads();
    *khi = st[3];
    __syncthreads();
  }
}

__global__ __launch_bounds__(TH_NT) void align_threshold_kernel(ArParams q) {
  __shared__ unsigned hist[256 * TH_COPIES];
  __shared__ unsigned st[4];
  __shared__ int bad;
  const int p = blockIdx.x, tid = threadIdx.x;
  ArHdr* h = q.hdr + p;
  const long long nl = ar_count(q, p);
  if (nl <= 0) {   // uniform: nothing selected (status 1), or a count the row cannot hold (status 2)
    if (tid == 0) { h->thr = NAN; h->ymed = NAN; h->flags = nl < 0 ? FLAG_BAD_SIZE : 0; h->m = 0; h->a_best = NAN; }
    return;
  }
  const int n = (int)nl;
  const float* x = q.x + (long long)p * q.stride;
  const float* y = q.y + (long long)p * q.stride;
  float2* xy = q.xy + (long long)p * q.stride;
  if (tid == 0) bad = 0;
  __syncthreads();
  int nf = 0;
#pragma unroll 4
  for (int i = tid; i < n; i += TH_NT) {
    const float xv = x[i], yv = y[i];
    nf |= (!finite_f32(xv) || !finite_f32(yv)) ? 1 : 0;
    xy[i] = make_float2(xv, yv);
  }
  if (nf) atomicOr(&bad, 1);
  __syncthreads();
  const long long m = ar_subset_size(q.min_samples, nl);
  int flags = bad ? FLAG_NONFINITE : 0;
  if (m < 1 || m > nl || (q.subsets && m > (long long)q.m_cap)) flags |= FLAG_BAD_SIZE;
  if (flags) {     // uniform: a failed fit (scikit-learn raises on a non-finite sample and on min_samples > n)
    if (tid == 0) { h->thr = NAN; h->ymed = NAN; h->flags = flags; h->m = 0; h->a_best = NAN; }
    return;
  }
  unsigned klo, khi;
  th_select<0>(y, n, 0.0f, hist, st, tid, &klo, &khi);
  const float med = (n & 1) ? ar_unkey(klo) : (ar_unkey(klo) + ar_unkey(khi)) / 2.0f;   // np.median: float32 mean of the middle values
  th_select<1>(y, n, med, hist, st, tid, &klo, &khi);
  const float thr = (n & 1) ? ar_unkey(klo) : (ar_unkey(klo) + ar_unkey(khi)) / 2.0f;
  if (tid == 0) { h->thr = thr; h->ymed = med; h->flags = 0; h->m = (int)m; h->a_best = NAN; }
}

// ---- subset sums ----------------------------------------------------------------------------------------------------------------
// float32(sum xy / sum xx) of one trial's subset; sum xx == 0 gives 0 (the minimum-norm solution lstsq returns)
__device__ inline float ar_slope(double sxy, double sxx) { return sxx == 0.0 ? 0.0f : (float)(sxy / sxx); }

__global__ __launch_bounds__(AR_NT) void align_subset_sums_kernel(ArParams q) {
  __shared__ double red[2 * AR_ROWS];
  __shared__ int oob;
  // the T workgroups of a frame gather from the same 8 n bytes: consecutive work items share an XCD, and so its L2 (xcd_remap)
  const int w = xcd_remap(blockIdx.x, gridDim.x), p = w / q.T, t = w - p * q.T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  ArHdr* h = q.hdr + p;
  const long long nl = ar_count(q, p);
  if (nl <= 0 || (h->flags & (FLAG_NONFINITE | FLAG_BAD_SIZE))) return;
  const int n = (int)nl, m = h->m;
  const float2* xy = q.xy + (long long)p * q.stride;
  const int* sub = q.subsets ? q.subsets + ((long long)p * q.T + t) * q.m_cap : nullptr;
  if (tid == 0) oob = 0;
  __syncthreads();
  double sxy = 0.0, sxx = 0.0;
  int bad = 0;
#pragma unroll 4
  for (int i = tid; i < m; i += AR_NT) {
    const int idx = sub ? sub[i] : ar_subset_index(q.seed, p, t, n, i);
    if ((unsigned)idx >= (unsigned)n) { bad = 1; continue; }   // checked before it addresses anything
    const float2 v = xy[idx];
    const double xv = (double)v.x, yv = (double)v.y;
    sxy += xv * yv;
    sxx += xv * xv;
  }
  if (bad) atomicOr(&oob, 1);
  sxy = wave_sum(sxy);
  sxx = wave_sum(sxx);
  if (lane == 0) { red[wave] = sxy; red[AR_ROWS + wave] = sxx; }
  __syncthreads();
  if (tid == 0) {
    const double a = (red[0] + red[1]) + (red[2] + red[3]), b = (red[AR_ROWS] + red[AR_ROWS + 1]) + (red[AR_ROWS + 2] + red[AR_ROWS + 3]);
    q.slopes[(long long)p * q.T + t] = ar_slope(a, b);
    if (oob) atomicOr(&h->flags, FLAG_BAD_INDEX);
  }
}

// the subsets a seed gives, i32 [P][T][m_cap]: the first m of a row are the draw, the rest -1 (la3d_align_ransac_subsets)
__global__ __launch_bounds__(AR_NT) void align_export_subsets_kernel(const long long* __restrict__ counts, double min_samples, int T, int m_cap,
                                                                      unsigned long long seed, int* __restrict__ out) {
  const int t = blockIdx.x, p = blockIdx.y;
  const long long nl = counts[p];
  long long m = (nl > 0 && nl <= (long long)LA3D_ALIGN_RANSAC_MAX_N) ? ar_subset_size(min_samples, nl) : 0;
  if (m < 1 || m > nl) m = 0;
  int* row = out + ((long long)p * T + t) * m_cap;
  for (int i = threadIdx.x; i < m_cap; i += AR_NT) row[i] = i < m ? ar_subset_index(seed, p, t, (int)nl, i) : -1;
}

// ---- the candidates pass --------------------------------------------------------------------------------------------------------
// inlier test of one sample under slope a: pred = float32(x * a) - ONE rounded product, never contracted into the subtraction -,
// r = y - pred in float32, |r| <= thr.  (`__fmul_rn` is a plain operation for hipcc and gets fused: the pragma is what holds.)
__device__ inline bool ar_inlier(float x, float y, float a, float thr, float* r_out) {
  float r;
  {
#pragma clang fp contract(off)
    const float pred = x * a;
    r = y - pred;
  }
  *r_out = r;
  return fabsf(r) <= thr;
}

__device__ inline float wave_min_f(float v) {
  v = fminf(v, __int_as_float(dpp_i32<DPP_XOR1>(__float_as_int(v))));
  v = fminf(v, __int_as_float(dpp_i32<DPP_XOR2>(__float_as_int(v))));
  v = fminf(v, __int_as_float(dpp_i32<DPP_HALF_MIRROR>(__float_as_int(v))));
  v = fminf(v, __int_as_float(dpp_i32<DPP_MIRROR>(__float_as_int(v))));
  return fminf(fminf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16))),
               fminf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48))));
}

// Each thread keeps its 16 samples in registers and walks the T slopes (LDS, read wave-uniformly); a wave reduces its 1024 samples per
// trial by DPP and leaves the result in its own LDS row - no barrier in the loop.  After one barrier the four rows are added in their
// fixed order and the segment's row of T partials leaves with coalesced stores; the scan kernel merges the segments in order.
// Dynamic LDS: T slopes, then [4 waves][T] of (three float64 sums; k, min, max).
__global__ __launch_bounds__(AR_NT) void align_candidates_kernel(ArParams q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int T = q.T;
  double* w_sy = reinterpret_cast<double*>(smem);          // [AR_ROWS][T]
  double* w_syy = w_sy + AR_ROWS * T;
  double* w_srr = w_syy + AR_ROWS * T;
  int* w_k = reinterpret_cast<int*>(w_srr + AR_ROWS * T);  // [AR_ROWS][T]
  float* w_mn = reinterpret_cast<float*>(w_k + AR_ROWS * T);
  float* w_mx = w_mn + AR_ROWS * T;
  float* s_slope = w_mx + AR_ROWS * T;                     // [T]
  const int seg = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ArHdr* h = q.hdr + p;
  const long long nl = ar_count(q, p);
  if (nl <= 0 || (long long)seg * AR_SEG >= nl || h->flags) return;
  const int n = (int)nl;
  const float* x = q.x + (long long)p * q.stride;
  const float* y = q.y + (long long)p * q.stride;
  const float thr = h->thr;
  const double ymed = (double)h->ymed;
  for (int t = tid; t < T; t += AR_NT) s_slope[t] = q.slopes[(long long)p * T + t];
  float xs[AR_PER], ys[AR_PER];
  double yd[AR_PER];
#pragma unroll
  for (int k = 0; k < AR_PER; ++k) {
    const int i = seg * AR_SEG + k * AR_NT + tid;
    xs[k] = i < n ? x[i] : 0.0f;
    ys[k] = i < n ? y[i] : NAN;          // past the end: never an inlier
    yd[k] = (double)ys[k] - ymed;        // the scores' sums run about the frame's median: no cancellation in sum y^2 - (sum y)^2 / k
  }
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const float a = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s_slope[t])));
    int k = 0;
    float mn = INFINITY, mx = -INFINITY;
    double sy = 0.0, syy = 0.0, srr = 0.0;
#pragma unroll
    for (int j = 0; j < AR_PER; ++j) {
      float r;
      const bool in = ar_inlier(xs[j], ys[j], a, thr, &r);
      const double ydm = in ? yd[j] : 0.0, rd = (double)(in ? r : 0.0f);
      k += in ? 1 : 0;
      sy += ydm;
      syy = fma(ydm, ydm, syy);
      srr = fma(rd, rd, srr);
      mn = fminf(mn, in ? ys[j] : INFINITY);
      mx = fmaxf(mx, in ? ys[j] : -INFINITY);
    }
    k = wave_sum_i(k);
    sy = wave_sum(sy); syy = wave_sum(syy); srr = wave_sum(srr);
    mn = wave_min_f(mn); mx = -wave_min_f(-mx);
    if (lane == 0) {
      const int o = wave * T + t;
      w_k[o] = k; w_mn[o] = mn; w_mx[o] = mx; w_sy[o] = sy; w_syy[o] = syy; w_srr[o] = srr;
    }
  }
  __syncthreads();
  const long long row = ((long long)p * q.rows + seg) * T;
  for (int t = tid; t < T; t += AR_NT) {
    q.pk[row + t] = (w_k[t] + w_k[T + t]) + (w_k[2 * T + t] + w_k[3 * T + t]);
    q.pmn[row + t] = fminf(fminf(w_mn[t], w_mn[T + t]), fminf(w_mn[2 * T + t], w_mn[3 * T + t]));
    q.pmx[row + t] = fmaxf(fmaxf(w_mx[t], w_mx[T + t]), fmaxf(w_mx[2 * T + t], w_mx[3 * T + t]));
    q.psy[row + t] = (w_sy[t] + w_sy[T + t]) + (w_sy[2 * T + t] + w_sy[3 * T + t]);
    q.psyy[row + t] = (w_syy[t] + w_syy[T + t]) + (w_syy[2 * T + t] + w_syy[3 * T + t]);
    q.psrr[row + t] = (w_srr[t] + w_srr[T + t]) + (w_srr[2 * T + t] + w_srr[3 * T + t]);
  }
}

// ---- trial scan -----------------------------------------------------------------------------------------------------------------
// scikit-learn's _dynamic_max_trials in float64
__device__ inline double ar_dynamic_max_trials(int k, int n, int m, double probability) {
  const double eps = 2.220446049250313e-16;   // np.spacing(1)
  const double ratio = (double)k / (double)n;
  const double nom = fmax(eps, 1.0 - probability);
  const double denom = fmax(eps, 1.0 - pow(ratio, (double)m));
  if (nom == 1.0) return 0.0;
  if (denom == 1.0) return INFINITY;
  return fabs(ceil(log(nom) / log(denom)));
}

// R^2 over the inliers with scikit-learn's special values: fewer than two samples NaN; zero total variance (all inlier y equal:
// min == max) 1 if the residual sum is 0, else 0.  sy, syy: sums of (y - c) and (y - c)^2 about the frame's median c.
__device__ inline double ar_score(int k, double sy, double syy, double srr, float mn, float mx) {
  if (k < 2) return NAN;
  if (mn == mx) return srr == 0.0 ? 1.0 : 0.0;
  const double den = syy - sy * sy / (double)k;
  return 1.0 - srr / den;
}

// Waves 0..3 each sum a fixed quarter of the frame's segment rows, lane = trial within a chunk of 64; wave 0 adds the four in order, scores
// the chunk and keeps (k, score) of every trial in LDS; then one thread walks the trials in order.
__global__ __launch_bounds__(AR_NT) void align_scan_trials_kernel(ArParams q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* s_score = reinterpret_cast<double*>(smem);            // [T]
  int* s_k = reinterpret_cast<int*>(s_score + q.T);             // [T]
  __shared__ double c_sy[AR_ROWS][64], c_syy[AR_ROWS][64], c_srr[AR_ROWS][64];
  __shared__ float c_mn[AR_ROWS][64], c_mx[AR_ROWS][64];
  __shared__ int c_k[AR_ROWS][64];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = q.T;
  ArHdr* h = q.hdr + p;
  const long long nl = ar_count(q, p);
  const int flags = h->flags;
  if (nl <= 0 || flags) {   // uniform
    if (tid == 0) {
      q.status[p] = (nl == 0) ? 1 : 2;
      q.coef[p] = NAN; q.n_inliers[p] = 0; q.n_trials[p] = 0; q.best_trial[p] = -1;
    }
    return;
  }
  const int n = (int)nl, m = h->m;
  const int rows = (n + AR_SEG - 1) / AR_SEG, rq = (rows + AR_ROWS - 1) / AR_ROWS;   // one row per segment, rq of them per wave
  const long long base = (long long)p * q.rows * T;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    int k = 0;
    float mn = INFINITY, mx = -INFINITY;
    double sy = 0.0, syy = 0.0, srr = 0.0;
    if (t < T) {
#pragma unroll 4
      for (int r = wave * rq; r < min((wave + 1) * rq, rows); ++r) {
        const long long o = base + (long long)r * T + t;
        k += q.pk[o];
        mn = fminf(mn, q.pmn[o]); mx = fmaxf(mx, q.pmx[o]);
        sy += q.psy[o]; syy += q.psyy[o]; srr += q.psrr[o];
      }
    }
    c_k[wave][lane] = k; c_mn[wave][lane] = mn; c_mx[wave][lane] = mx;
    c_sy[wave][lane] = sy; c_syy[wave][lane] = syy; c_srr[wave][lane] = srr;
    __syncthreads();
    if (wave == 0 && t < T) {
      const int kk = (c_k[0][lane] + c_k[1][lane]) + (c_k[2][lane] + c_k[3][lane]);
      const float a = fminf(fminf(c_mn[0][lane], c_mn[1][lane]), fminf(c_mn[2][lane], c_mn[3][lane]));
      const float b = fmaxf(fmaxf(c_mx[0][lane], c_mx[1][lane]), fmaxf(c_mx[2][lane], c_mx[3][lane]));
      const double s1 = (c_sy[0][lane] + c_sy[1][lane]) + (c_sy[2][lane] + c_sy[3][lane]);
      const double s2 = (c_syy[0][lane] + c_syy[1][lane]) + (c_syy[2][lane] + c_syy[3][lane]);
      const double s3 = (c_srr[0][lane] + c_srr[1][lane]) + (c_srr[2][lane] + c_srr[3][lane]);
      s_k[t] = kk;
      s_score[t] = ar_score(kk, s1, s2, s3, a, b);
    }
    __syncthreads();
  }
  if (tid == 0) {   // scikit-learn's loop (RANSACRegressor.fit): NaN scores compare false, as there
    int k_best = 1, best = -1, t = 0;
    double score_best = -INFINITY, limit = (double)T;
    while ((double)t < limit) {
      const int kt = s_k[t];
      const double sc = s_score[t];
      ++t;
      if (kt < k_best) continue;
      if (kt == k_best && sc < score_best) continue;
      k_best = kt; score_best = sc; best = t - 1;
      limit = fmin(limit, ar_dynamic_max_trials(k_best, n, m, q.stop_probability));
    }
    q.n_trials[p] = t;
    q.best_trial[p] = best;
    q.n_inliers[p] = best >= 0 ? k_best : 0;
    q.status[p] = best >= 0 ? 0 : 2;
    q.coef[p] = NAN;                                 // the finish kernel writes it
    h->a_best = best >= 0 ? q.slopes[(long long)p * T + best] : NAN;
  }
}

// ---- refit ----------------------------------------------------------------------------------------------------------------------
// sum xy, sum xx over the inliers of the best slope (the test is recomputed: no mask is stored), one pair per segment
__global__ __launch_bounds__(AR_NT) void align_refit_kernel(ArParams q) {
  __shared__ double red[2 * AR_ROWS];
  const int seg = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ArHdr* h = q.hdr + p;
  const long long nl = ar_count(q, p);
  if (nl <= 0 || (long long)seg * AR_SEG >= nl || q.status[p] != 0) return;
  const int n = (int)nl;
  const float* x = q.x + (long long)p * q.stride;
  const float* y = q.y + (long long)p * q.stride;
  const float thr = h->thr, a = h->a_best;
  double sxy = 0.0, sxx = 0.0;
#pragma unroll
  for (int k = 0; k < AR_PER; ++k) {
    const int i = seg * AR_SEG + k * AR_NT + tid;
    const float xv = i < n ? x[i] : 0.0f, yv = i < n ? y[i] : NAN;
    float r;
    if (ar_inlier(xv, yv, a, thr, &r)) {
      sxy += (double)xv * (double)yv;
      sxx += (double)xv * (double)xv;
    }
  }
  sxy = wave_sum(sxy);
  sxx = wave_sum(sxx);
  if (lane == 0) { red[wave] = sxy; red[AR_ROWS + wave] = sxx; }
  __syncthreads();
  if (tid == 0) {
    double* o = q.rf + ((long long)p * q.nseg + seg) * 2;
    o[0] = (red[0] + red[1]) + (red[2] + red[3]);
    o[1] = (red[AR_ROWS] + red[AR_ROWS + 1]) + (red[AR_ROWS + 2] + red[AR_ROWS + 3]);
  }
}

__global__ __launch_bounds__(64) void align_finish_kernel(ArParams q) {
  const int p = blockIdx.x, lane = threadIdx.x;
  if (q.status[p] != 0) return;
  const int nseg = (int)((ar_count(q, p) + AR_SEG - 1) / AR_SEG);
  const double* o = q.rf + (long long)p * q.nseg * 2;
  double sxy = 0.0, sxx = 0.0;
  for (int s = lane; s < nseg; s += 64) { sxy += o[2 * s]; sxx += o[2 * s + 1]; }
  sxy = wave_sum(sxy);
  sxx = wave_sum(sxx);
  if (lane == 0) q.coef[p] = ar_slope(sxy, sxx);
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------
// out = full(fill); out[sel] = float32(relative * coef), sel = mask if given else ~isinf(relative) - the expression of
// align_apply_kernel (la3d_consumers.hip) with the fitted coefficient read from the device; a frame that was not fitted gets its metric
// depth, which is what the reference returns for it
__global__ __launch_bounds__(256) void align_apply_batch_kernel(const float* __restrict__ rel, const float* __restrict__ met,
                                                                const unsigned char* __restrict__ mask, long long n,
                                                                const float* __restrict__ coef, const int* __restrict__ status,
                                                                float intercept, float fill, float* __restrict__ out) {
  const int p = blockIdx.y;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long g = (long long)p * n + i;
  if (status[p] != 0) { out[g] = met[g]; return; }
  const float c = coef[p];
  const float r = rel[g];
  const bool sel = mask ? mask[g] != 0 : (__float_as_uint(r) & 0x7fffffffu) != 0x7f800000u;
  float v;
  {
#pragma clang fp contract(off)
    const float prod = r * c;
    v = prod + intercept;
  }
  out[g] = sel ? v : fill;
}

const char* ar_check(const la3d_align_ransac_args* a, int* rc) {
  *rc = LA3D_ERR_ARG;
  if (!a) return "NULL argument block";
  if (a->struct_size != (int32_t)sizeof(la3d_align_ransac_args)) return "struct_size is not sizeof(la3d_align_ransac_args)";
  if (a->P < 0 || a->n < 0) return "negative P or n";
  if (a->max_trials < 1) return "max_trials must be at least 1";
  if (!(a->min_samples > 0.0) || (a->min_samples >= 1.0 && (a->min_samples != (double)(long long)a->min_samples || a->min_samples > 2147483647.0)))
    return "min_samples must be a fraction in (0, 1) or an integer >= 1";
  if (!(a->stop_probability >= 0.0 && a->stop_probability <= 1.0)) return "stop_probability outside [0, 1]";
  if (a->subsets && a->m_cap < 1) return "subsets given with m_cap < 1";
  if ((reinterpret_cast<uintptr_t>(a->relative_sel) | reinterpret_cast<uintptr_t>(a->metric_sel) | reinterpret_cast<uintptr_t>(a->subsets) |
       reinterpret_cast<uintptr_t>(a->coef) | reinterpret_cast<uintptr_t>(a->n_inliers) | reinterpret_cast<uintptr_t>(a->n_trials) |
       reinterpret_cast<uintptr_t>(a->best_trial) | reinterpret_cast<uintptr_t>(a->status)) & 3u)
    return "a pointer is not 4-byte aligned";
  if ((reinterpret_cast<uintptr_t>(a->counts) & 7u) || (reinterpret_cast<uintptr_t>(a->workspace) & 15u))
    return "counts must be 8-byte, the workspace 16-byte aligned";
  if (a->P > 0 && (!a->counts || !a->coef || !a->n_inliers || !a->n_trials || !a->best_trial || !a->status || !a->workspace ||
                   (a->n > 0 && (!a->relative_sel || !a->metric_sel))))
    return "NULL pointer with work to do";
  *rc = LA3D_ERR_UNSUPPORTED;
  if (a->n > LA3D_ALIGN_RANSAC_MAX_N) return "more than LA3D_ALIGN_RANSAC_MAX_N samples per frame";
  if (a->max_trials > LA3D_ALIGN_RANSAC_MAX_TRIALS) return "more than LA3D_ALIGN_RANSAC_MAX_TRIALS trials";
  if (a->P > 65535) return "more than 65535 frames";
  *rc = LA3D_SUCCESS;
  return nullptr;
}

}  // namespace

extern "C" {

size_t la3d_align_ransac_workspace_bytes(int P, int64_t n, int max_trials) {
  if (P <= 0 || n < 0 || max_trials < 1 || n > LA3D_ALIGN_RANSAC_MAX_N || max_trials > LA3D_ALIGN_RANSAC_MAX_TRIALS) return 16;
  return ar_layout(P, n, max_trials).total;
}

int la3d_align_ransac_batch(const la3d_align_ransac_args* a) {
  int rc;
  if (const char* what = ar_check(a, &rc)) return refuse("la3d_align_ransac_batch", what, rc);
  if (a->P == 0) return LA3D_SUCCESS;
  const int P = a->P, T = a->max_trials;
  const ArLayout L = ar_layout(P, a->n, T);
  unsigned char* ws = static_cast<unsigned char*>(a->workspace);
  ArParams q;
  q.x = a->relative_sel; q.y = a->metric_sel; q.counts = reinterpret_cast<const long long*>(a->counts);
  q.stride = a->n;
  q.min_samples = a->min_samples; q.stop_probability = a->stop_probability;
  q.T = T; q.m_cap = a->m_cap;
  q.subsets = a->subsets;
  q.seed = a->seed;
  q.coef = a->coef; q.n_inliers = a->n_inliers; q.n_trials = a->n_trials; q.best_trial = a->best_trial; q.status = a->status;
  q.hdr = reinterpret_cast<ArHdr*>(ws + L.hdr);
  q.slopes = reinterpret_cast<float*>(ws + L.slopes);
  q.xy = reinterpret_cast<float2*>(ws + L.xy);
  q.pk = reinterpret_cast<int*>(ws + L.pk);
  q.pmn = reinterpret_cast<float*>(ws + L.pmn); q.pmx = reinterpret_cast<float*>(ws + L.pmx);
  q.psy = reinterpret_cast<double*>(ws + L.psy); q.psyy = reinterpret_cast<double*>(ws + L.psyy); q.psrr = reinterpret_cast<double*>(ws + L.psrr);
  q.rf = reinterpret_cast<double*>(ws + L.rf);
  q.nseg = L.nseg; q.rows = L.rows;
  hipStream_t s = static_cast<hipStream_t>(a->stream);
  const unsigned nseg = (unsigned)L.nseg;
  hipLaunchKernelGGL(align_threshold_kernel, dim3(P), dim3(TH_NT), 0, s, q);
  hipLaunchKernelGGL(align_subset_sums_kernel, dim3((unsigned)T * (unsigned)P), dim3(AR_NT), 0, s, q);
  const size_t cand_lds = (size_t)T * (AR_ROWS * 36 + 4);   // at most 148 KiB (T = 1024)
  allow_big_lds(reinterpret_cast<const void*>(align_candidates_kernel));
  hipLaunchKernelGGL(align_candidates_kernel, dim3(nseg, P), dim3(AR_NT), cand_lds, s, q);
  hipLaunchKernelGGL(align_scan_trials_kernel, dim3(P), dim3(AR_NT), (size_t)T * 12, s, q);
  hipLaunchKernelGGL(align_refit_kernel, dim3(nseg, P), dim3(AR_NT), 0, s, q);
  hipLaunchKernelGGL(align_finish_kernel, dim3(P), dim3(64), 0, s, q);
  return check_launch("la3d_align_ransac_batch");
}

int la3d_align_ransac_subsets(const int64_t* counts, int P, double min_samples, int max_trials, uint64_t seed, int32_t* subsets,
                              int m_cap, void* stream) {
  if (P < 0 || max_trials < 1 || m_cap < 1 || !(min_samples > 0.0) ||
      (min_samples >= 1.0 && (min_samples != (double)(long long)min_samples || min_samples > 2147483647.0)) ||
      (P > 0 && (!counts || !subsets)) || (reinterpret_cast<uintptr_t>(counts) & 7u) || (reinterpret_cast<uintptr_t>(subsets) & 3u))
    return refuse("la3d_align_ransac_subsets", "bad argument");
  if (max_trials > LA3D_ALIGN_RANSAC_MAX_TRIALS || P > 65535)
    return refuse("la3d_align_ransac_subsets", "more than LA3D_ALIGN_RANSAC_MAX_TRIALS trials or 65535 frames", LA3D_ERR_UNSUPPORTED);
  if (P == 0) return LA3D_SUCCESS;
  hipLaunchKernelGGL(align_export_subsets_kernel, dim3(max_trials, P), dim3(AR_NT), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(counts), min_samples, max_trials, m_cap, (unsigned long long)seed, subsets);
  return check_launch("la3d_align_ransac_subsets");
}

int la3d_align_apply_batch(const float* relative, const float* metric, const uint8_t* mask, int P, int64_t n, const float* coef,
                           const int32_t* status, float fill, float* out, void* stream) {
  if (P < 0 || P > 65535 || n < 0 || (P > 0 && n > 0 && (!relative || !metric || !coef || !status || !out)) ||
      ((reinterpret_cast<uintptr_t>(relative) | reinterpret_cast<uintptr_t>(metric) | reinterpret_cast<uintptr_t>(coef) |
        reinterpret_cast<uintptr_t>(status) | reinterpret_cast<uintptr_t>(out)) & 3u))
    return refuse("la3d_align_apply_batch", "bad argument (P <= 65535, 4-byte aligned pointers)");
  if (P == 0 || n == 0) return LA3D_SUCCESS;
  if ((n + 255) / 256 > 0x7fffffffLL) return refuse("la3d_align_apply_batch", "frame too large", LA3D_ERR_UNSUPPORTED);
  hipLaunchKernelGGL(align_apply_batch_kernel, dim3((unsigned)((n + 255) / 256), P), dim3(256), 0, static_cast<hipStream_t>(stream),
                     relative, metric, mask, (long long)n, coef, status, 0.0f, fill, out);
  return check_launch("la3d_align_apply_batch");
}

}  // extern "C"
