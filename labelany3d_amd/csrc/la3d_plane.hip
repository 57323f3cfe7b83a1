// la3d_plane.hip - the ground plane from the depth (include/la3d.h "ground plane: RANSAC plane fit"): the `ground` vector of the fit
// entries for P images of one size, as the dominant plane of their back-projected grid samples.  Two entries, each a linear chain of
// launches on the caller's stream without host synchronisation, allocation or read-back (restated in tests/ground_plane_cases.py).
//
// la3d_plane_select_batch, two launches:
//   count       one workgroup per 4096 grid pixels: the kept pixels of its chunk (ballot + popcount) -> the workspace
//   write       the same grid tests the same pixels again, ranks them - chunks before it from the workspace, then wave ballots in
//               raster order - and writes point (cloud_point: the row of la3d_unproject_batch) and pixel index; chunk 0 writes counts
// la3d_plane_ransac_batch, nine launches:
//   trials      one thread per (trial, frame): its three indices (given or drawn: la3d_draw.hpp), a, w = (b - a) x (c - a), s, the skips
//   candidates  one workgroup per 1024 samples: ONE sweep judges all T planes - samples in registers, planes in LDS read wave-uniformly,
//               counts by ballot + popcount, one integer row of T partials per segment
//   pick        one workgroup per frame: the segment rows added up, the largest k with the lowest t, the status
//   mean        one workgroup per 1024 samples: sum x, y, z over the inliers of the best trial
//   centre      one wave per frame: mu from the segment sums, in fixed order
//   covariance  one workgroup per 1024 samples: the six sums of products ABOUT mu over the same inliers
//   refit       one wave per frame: the covariance from the segment sums, its smallest eigenvector (cyclic Jacobi), orientation, d
//   recount     one workgroup per 1024 samples: residuals under the reported plane, final flags, count and sum r^2 per segment
//   report      one wave per frame: n_inliers, rms
// No floating-point atomics: every float sum is merged in a fixed order (thread -> wave butterfly -> the four waves -> the segments),
// and the order depends on the frame's own count only, so a frame's result is the same alone and in any batch.
#include <cstddef>
#include <cstdint>

#include "la3d_device.hpp"
#include "la3d_draw.hpp"
#include "la3d_point.hpp"

using namespace la3d;

// every product and sum below is rounded on its own, in the order written (the headers above keep the default)
#pragma clang fp contract(off)

namespace {

// ---- select ---------------------------------------------------------------------------------------------------------------------
constexpr int PS_NT = 256;                 // threads per workgroup
constexpr int PS_PER = 16;                 // grid pixels per thread
constexpr int PS_CHUNK = PS_NT * PS_PER;   // grid pixels per workgroup (4096)
constexpr int PS_WAVES = PS_NT / 64;

struct PsParams {
  int P, H, W, step, gw, cap, nchunk, k_stride;
  float near_d, far_d;
  const float* depth;
  const double* K;
  const unsigned* cand;
  long long cand_stride;     // words
  int cand_width;
  double* points;
  int* pixel;
  long long* counts;
  int* ws;                   // [P][nchunk] kept pixels per chunk
};

// the chunk's 16 grid pixels of this thread: bit k of the result = pixel k * 256 + tid of the chunk is kept; d[k] its depth
__device__ inline unsigned ps_flags(const PsParams& q, int p, int chunk, int tid, float* d) {
  const float* dp = q.depth + (long long)p * q.H * q.W;
  const unsigned* cp = q.cand ? q.cand + (long long)p * q.cand_stride : nullptr;
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < PS_PER; ++k) {
    const int g = chunk * PS_CHUNK + k * PS_NT + tid;
    d[k] = 0.0f;
    if (g < q.cap) {
      const int gv = g / q.gw, v = gv * q.step, u = (g - gv * q.gw) * q.step;
      const float dv = dp[(long long)v * q.W + u];
      d[k] = dv;
      // finite and > 0 on the bit pattern - a subnormal depth is a depth whatever the denormal mode -, then the two float32 comparisons
      bool keep = __float_as_uint(dv) - 1u < 0x7f7fffffu && q.near_d <= dv && dv <= q.far_d;
      if (keep && cp) {
        const long long b = (long long)v * q.cand_width + u;
        keep = (cp[b >> 5] >> (b & 31)) & 1u;
      }
      m |= keep ? (1u << k) : 0u;
    }
  }
  return m;
}

__global__ __launch_bounds__(PS_NT) void plane_select_count_kernel(PsParams q) {
  __shared__ int wcnt[PS_WAVES];
  const int chunk = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float d[PS_PER];
  const unsigned m = ps_flags(q, p, chunk, tid, d);
  int c = 0;
#pragma unroll
  for (int k = 0; k < PS_PER; ++k) c += __popcll(__ballot((m >> k) & 1u));
  if (lane == 0) wcnt[wave] = c;
  __syncthreads();
  if (tid == 0) q.ws[(long long)p * q.nchunk + chunk] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
}

__global__ __launch_bounds__(PS_NT) void plane_select_write_kernel(PsParams q) {
  __shared__ double kinv[9];
  __shared__ int cnt[PS_PER * PS_WAVES], excl[PS_PER * PS_WAVES], red[2 * PS_WAVES];
  const int chunk = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0 && q.cap > 0) inv3(q.K + (long long)p * q.k_stride, kinv);
  float d[PS_PER];
  const unsigned m = ps_flags(q, p, chunk, tid, d);
  // kept pixels in the chunks before this one (integers: any order), and - chunk 0 - in the whole image
  const int* wsp = q.ws + (long long)p * q.nchunk;
  int before = 0, all = 0;
  for (int c = tid; c < chunk; c += PS_NT) before += wsp[c];
  if (chunk == 0)
    for (int c = tid; c < q.nchunk; c += PS_NT) all += wsp[c];
  before = wave_sum_i(before);
  all = wave_sum_i(all);
  if (lane == 0) { red[wave] = before; red[PS_WAVES + wave] = all; }
#pragma unroll
  for (int k = 0; k < PS_PER; ++k) {
    const int c = __popcll(__ballot((m >> k) & 1u));
    if (lane == 0) cnt[k * PS_WAVES + wave] = c;
  }
  __syncthreads();
  if (wave == 0) {   // raster order inside the chunk: k, then wave, then lane - an exclusive scan over the 64 (k, wave) counts
    const int mine = cnt[lane];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    excl[lane] = incl - mine;
  }
  __syncthreads();
  const long long base = (red[0] + red[1]) + (red[2] + red[3]);
  if (chunk == 0 && tid == 0) q.counts[p] = (long long)((red[PS_WAVES] + red[PS_WAVES + 1]) + (red[PS_WAVES + 2] + red[PS_WAVES + 3]));
  double* pts = q.points + (long long)p * q.cap * 3;
  int* pix = q.pixel + (long long)p * q.cap;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < PS_PER; ++k) {
    const unsigned long long bal = __ballot((m >> k) & 1u);
    if ((m >> k) & 1u) {
      const int g = chunk * PS_CHUNK + k * PS_NT + tid;
      const int gv = g / q.gw, v = gv * q.step, u = (g - gv * q.gw) * q.step;
      const long long r = base + excl[k * PS_WAVES + wave] + __popcll(bal & below);   // < cap: a rank among the kept grid pixels
      double w[3];
      cloud_point((double)d[k], (unsigned)u, (unsigned)v, kinv, w);
      pts[r * 3] = w[0]; pts[r * 3 + 1] = w[1]; pts[r * 3 + 2] = w[2];
      pix[r] = v * q.W + u;
    }
  }
}

// ---- RANSAC ---------------------------------------------------------------------------------------------------------------------
constexpr int PR_NT = 256;                       // threads of the sample-parallel kernels
constexpr int PR_PER = 4;                        // samples per thread
constexpr int PR_SEG = PR_NT * PR_PER;           // samples per workgroup
constexpr int PR_ROWS = PR_NT / 64;              // waves per workgroup
constexpr int PR_TW = 8;                         // doubles of a trial in the workspace: a[3], w[3], s, accepted (1 / 0)
constexpr int PR_TL = 7;                         // doubles of a trial in LDS
static_assert(PR_SEG == LA3D_PLANE_SEGMENT, "include/la3d.h states the segment");

// per-frame header in the workspace
struct PrHdr {
  double a[3], w[3], s;     // the best trial
  double mu[3];
  double plane[4];          // as reported
  int status, best, k, count;
};

struct PrLayout {
  long long nseg;
  size_t hdr, trials, pk, pm, pc, prr, prk, total;
};
inline size_t pr_up16(size_t v) { return (v + 15) & ~(size_t)15; }
inline PrLayout pr_layout(long long P, long long n, long long T) {
  PrLayout L;
  L.nseg = n > 0 ? (n + PR_SEG - 1) / PR_SEG : 1;
  const size_t seg = (size_t)P * (size_t)L.nseg;
  size_t o = 0;
  L.hdr = o; o = pr_up16(o + (size_t)P * sizeof(PrHdr));
  L.trials = o; o = pr_up16(o + (size_t)P * T * PR_TW * 8);
  L.pk = o; o = pr_up16(o + seg * T * 4);
  L.pm = o; o = pr_up16(o + seg * 3 * 8);
  L.pc = o; o = pr_up16(o + seg * 6 * 8);
  L.prr = o; o = pr_up16(o + seg * 8);
  L.prk = o; o = pr_up16(o + seg * 4);
  L.total = o;
  return L;
}

struct PrParams {
  const double* pts;
  const long long* counts;
  long long stride;          // samples between frames (the capacity n of a row)
  double thr_abs, thr_rel, cos2_tilt;
  int T, min_inliers;
  const int* subsets;
  unsigned long long seed;
  double* plane;
  int *k_trial, *n_inliers, *best_trial, *status;
  double* rms;
  unsigned char* inliers;
  PrHdr* hdr;
  double* trials;            // [P][T][PR_TW]
  int* pk;                   // [P][nseg][T]
  double *pm, *pc, *prr;     // [P][nseg][3], [6], [1]
  int* prk;                  // [P][nseg]
  long long nseg;
};

__device__ inline bool finite_f64(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// samples of frame p: its count when it fits the row, -1 otherwise (status 3, before anything is addressed by it)
__device__ inline long long pr_count(const PrParams& q, int p) {
  const long long c = q.counts[p];
  return (c < 0 || c > q.stride) ? -1 : c;
}

// sample i of a frame: coordinates and tol = thr_abs + thr_rel * z.  Past the end, or with a non-finite coordinate, tol is NaN - no test
// of the sample is ever true - and the coordinates are 0.
struct PrSample { double x, y, z, tol; };
__device__ inline PrSample pr_sample(const double* __restrict__ pts, int i, int n, double thr_abs, double thr_rel) {
  PrSample s;
  s.x = 0.0; s.y = 0.0; s.z = 0.0; s.tol = NAN;
  if (i < n) {
    const double x = pts[(long long)i * 3], y = pts[(long long)i * 3 + 1], z = pts[(long long)i * 3 + 2];
    if (finite_f64(x) && finite_f64(y) && finite_f64(z)) {
      const double rel = thr_rel * z;
      s.x = x; s.y = y; s.z = z; s.tol = thr_abs + rel;
    }
  }
  return s;
}

// the inlier test of a trial: e e <= (tol tol) s, with tol2 = tol * tol handed in
__device__ inline bool pr_inlier(const PrSample& q, double tol2, const double* a, const double* w, double s) {
  const double dx = q.x - a[0], dy = q.y - a[1], dz = q.z - a[2];
  const double e = (w[0] * dx + w[1] * dy) + w[2] * dz;
  return e * e <= tol2 * s;
}

// ---- trials ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PR_NT) void plane_trials_kernel(PrParams q) {
  const int t = blockIdx.x * PR_NT + threadIdx.x, p = blockIdx.y;
  if (t >= q.T) return;
  double* o = q.trials + ((long long)p * q.T + t) * PR_TW;
  const long long nl = pr_count(q, p);
  double a[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0}, s = NAN;
  bool ok = false;
  if (nl >= 3) {
    const int n = (int)nl;
    int idx[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) idx[i] = q.subsets ? q.subsets[((long long)p * q.T + t) * 3 + i] : ar_subset_index(q.seed, p, t, n, i);
    if ((unsigned)idx[0] < (unsigned)n && (unsigned)idx[1] < (unsigned)n && (unsigned)idx[2] < (unsigned)n) {   // checked before they address anything
      const double* fp = q.pts + (long long)p * q.stride * 3;
      const double* pa = fp + (long long)idx[0] * 3;
      const double* pb = fp + (long long)idx[1] * 3;
      const double* pc = fp + (long long)idx[2] * 3;
      a[0] = pa[0]; a[1] = pa[1]; a[2] = pa[2];
      const double ux = pb[0] - a[0], uy = pb[1] - a[1], uz = pb[2] - a[2];
      const double vx = pc[0] - a[0], vy = pc[1] - a[1], vz = pc[2] - a[2];
      w[0] = uy * vz - uz * vy;
      w[1] = uz * vx - ux * vz;
      w[2] = ux * vy - uy * vx;
      s = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
      ok = s > 0.0 && finite_f64(s) && w[1] * w[1] >= q.cos2_tilt * s;
    }
  }
  if (!ok) { a[0] = a[1] = a[2] = 0.0; w[0] = w[1] = w[2] = 0.0; s = NAN; }   // (a NaN s: no sample passes the test of a skipped trial)
  o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = w[0]; o[4] = w[1]; o[5] = w[2]; o[6] = s; o[7] = ok ? 1.0 : 0.0;
}

// ---- the candidates pass --------------------------------------------------------------------------------------------------------
// Each thread keeps its 4 samples in registers and walks the T planes (LDS, every lane reads the same address: a broadcast); a wave
// counts the inliers of its 256 samples per trial by ballot + popcount - scalar work - and leaves the count in its own LDS row, no barrier
// in the loop.  After one barrier the four rows are added and the segment's row of T integer partials leaves with coalesced stores.
// Dynamic LDS: [T][7] doubles, then [4 waves][T] ints.
__global__ __launch_bounds__(PR_NT) void plane_candidates_kernel(PrParams q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int T = q.T;
  double* s_tr = reinterpret_cast<double*>(smem);                  // [T][PR_TL]
  int* w_k = reinterpret_cast<int*>(s_tr + (size_t)T * PR_TL);     // [PR_ROWS][T]
  const int seg = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long nl = pr_count(q, p);
  if (nl < 3 || (long long)seg * PR_SEG >= nl) return;             // uniform
  const int n = (int)nl;
  const double* tr = q.trials + (long long)p * T * PR_TW;
  for (int i = tid; i < T * PR_TL; i += PR_NT) {
    const int t = i / PR_TL, c = i - t * PR_TL;
    s_tr[i] = tr[t * PR_TW + c];
  }
  const double* pts = q.pts + (long long)p * q.stride * 3;
  PrSample sm[PR_PER];
  double tol2[PR_PER];
#pragma unroll
  for (int k = 0; k < PR_PER; ++k) {
    sm[k] = pr_sample(pts, seg * PR_SEG + k * PR_NT + tid, n, q.thr_abs, q.thr_rel);
    tol2[k] = sm[k].tol * sm[k].tol;
  }
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const double* c = s_tr + t * PR_TL;
    const double a[3] = {c[0], c[1], c[2]}, w[3] = {c[3], c[4], c[5]};
    const double s = c[6];
    int k = 0;
#pragma unroll
    for (int j = 0; j < PR_PER; ++j) k += __popcll(__ballot(pr_inlier(sm[j], tol2[j], a, w, s)));
    if (lane == 0) w_k[wave * T + t] = k;
  }
  __syncthreads();
  int* row = q.pk + ((long long)p * q.nseg + seg) * T;
  for (int t = tid; t < T; t += PR_NT) row[t] = (w_k[t] + w_k[T + t]) + (w_k[2 * T + t] + w_k[3 * T + t]);
}

// ---- pick -----------------------------------------------------------------------------------------------------------------------
// thread = trial: the segment rows added (integers), then the largest k with the lowest t by a tree over packed keys
__global__ __launch_bounds__(PR_NT) void plane_pick_kernel(PrParams q) {
  __shared__ long long key[PR_NT];
  const int p = blockIdx.x, tid = threadIdx.x, T = q.T;
  PrHdr* h = q.hdr + p;
  const long long nl = pr_count(q, p);
  long long best = -1;                                    // k << 10 | (1023 - t): larger k first, then the lower t
  if (nl >= 3) {
    const int rows = (int)((nl + PR_SEG - 1) / PR_SEG);
    const int* pk = q.pk + (long long)p * q.nseg * T;
    const double* tr = q.trials + (long long)p * T * PR_TW;
    for (int t = tid; t < T; t += PR_NT) {
      if (tr[t * PR_TW + 7] == 0.0) continue;
      long long k = 0;
      for (int r = 0; r < rows; ++r) k += pk[(long long)r * T + t];
      const long long kt = (k << 10) | (long long)(LA3D_PLANE_MAX_TRIALS - 1 - t);
      best = kt > best ? kt : best;
    }
  }
  key[tid] = best;
  __syncthreads();
  for (int o = PR_NT / 2; o > 0; o >>= 1) {
    if (tid < o && key[tid + o] > key[tid]) key[tid] = key[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const long long b = key[0];
    int st = 0, bt = -1, k = 0;
    if (nl < 0) st = 3;
    else if (nl < 3) st = 1;
    else if (b < 0) st = 2;
    else {
      bt = LA3D_PLANE_MAX_TRIALS - 1 - (int)(b & 1023);
      k = (int)(b >> 10);
      if (k < q.min_inliers) { st = 2; bt = -1; k = 0; }
    }
    h->status = st; h->best = bt; h->k = k; h->count = nl < 0 ? 0 : (int)nl;
    if (st == 0) {
      const double* c = q.trials + ((long long)p * T + bt) * PR_TW;
      h->a[0] = c[0]; h->a[1] = c[1]; h->a[2] = c[2]; h->w[0] = c[3]; h->w[1] = c[4]; h->w[2] = c[5]; h->s = c[6];
    }
    q.status[p] = st; q.best_trial[p] = bt; q.k_trial[p] = k;
    if (st != 0) {
      q.n_inliers[p] = 0; q.rms[p] = NAN;
#pragma unroll
      for (int i = 0; i < 4; ++i) { q.plane[(long long)p * 4 + i] = NAN; h->plane[i] = NAN; }
    }
  }
}

// the four wave results of a workgroup in their fixed order; red: [NV][PR_ROWS] doubles in LDS.  Ends with the values in thread 0.
template <int NV>
__device__ inline void pr_block_sum(double* v, double* red, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    v[i] = wave_sum(v[i]);
    if (lane == 0) red[i * PR_ROWS + wave] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = (red[i * PR_ROWS] + red[i * PR_ROWS + 1]) + (red[i * PR_ROWS + 2] + red[i * PR_ROWS + 3]);
}

// ---- mean, centre, covariance ---------------------------------------------------------------------------------------------------
// CENTRED = false: sum x, y, z over the inliers of the best trial; true: the six sums of products about mu (the test is recomputed:
// no flags are stored in between)
template <bool CENTRED>
__global__ __launch_bounds__(PR_NT) void plane_moments_kernel(PrParams q) {
  constexpr int NV = CENTRED ? 6 : 3;
  __shared__ double red[NV * PR_ROWS];
  const int seg = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  const PrHdr* h = q.hdr + p;
  if (h->status != 0 || (long long)seg * PR_SEG >= (long long)h->count) return;   // uniform
  const int n = h->count;
  const double a[3] = {h->a[0], h->a[1], h->a[2]}, w[3] = {h->w[0], h->w[1], h->w[2]};
  const double s = h->s, mx = CENTRED ? h->mu[0] : 0.0, my = CENTRED ? h->mu[1] : 0.0, mz = CENTRED ? h->mu[2] : 0.0;
  const double* pts = q.pts + (long long)p * q.stride * 3;
  double v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
#pragma unroll
  for (int k = 0; k < PR_PER; ++k) {
    const PrSample sm = pr_sample(pts, seg * PR_SEG + k * PR_NT + tid, n, q.thr_abs, q.thr_rel);
    const bool in = pr_inlier(sm, sm.tol * sm.tol, a, w, s);
    if (CENTRED) {
      const double dx = in ? sm.x - mx : 0.0, dy = in ? sm.y - my : 0.0, dz = in ? sm.z - mz : 0.0;
      v[0] += dx * dx; v[1] += dx * dy; v[2] += dx * dz; v[3] += dy * dy; v[4] += dy * dz; v[5] += dz * dz;
    } else {
      v[0] += in ? sm.x : 0.0; v[1] += in ? sm.y : 0.0; v[2] += in ? sm.z : 0.0;
    }
  }
  pr_block_sum<NV>(v, red, tid);
  if (tid == 0) {
    double* o = (CENTRED ? q.pc : q.pm) + ((long long)p * q.nseg + seg) * NV;
#pragma unroll
    for (int i = 0; i < NV; ++i) o[i] = v[i];
  }
}

// the segment sums of a frame in fixed order: lane l adds segments l, l + 64, ..., then the butterfly
template <int NV>
__device__ inline void pr_merge_segments(const double* part, int nseg, int lane, double* v) {
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
  for (int r = lane; r < nseg; r += 64)
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] += part[(long long)r * NV + i];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
}

__global__ __launch_bounds__(64) void plane_centre_kernel(PrParams q) {
  const int p = blockIdx.x, lane = threadIdx.x;
  PrHdr* h = q.hdr + p;
  if (h->status != 0) return;
  const int nseg = (h->count + PR_SEG - 1) / PR_SEG;
  double v[3];
  pr_merge_segments<3>(q.pm + (long long)p * q.nseg * 3, nseg, lane, v);
  if (lane == 0) {
    const double k = (double)h->k;
    h->mu[0] = v[0] / k; h->mu[1] = v[1] / k; h->mu[2] = v[2] / k;
  }
}

// ---- refit ----------------------------------------------------------------------------------------------------------------------
// one Jacobi rotation that annihilates A[P_][Q_] of the symmetric A; V collects the rotations (columns = eigenvectors)
template <int P_, int Q_>
__device__ inline void jacobi_rotate(double (&A)[3][3], double (&V)[3][3]) {
  constexpr int R_ = 3 - P_ - Q_;
  const double apq = A[P_][Q_];
  if (apq == 0.0) return;
  const double theta = (A[Q_][Q_] - A[P_][P_]) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double arp = A[R_][P_], arq = A[R_][Q_];
  A[P_][P_] -= t * apq;
  A[Q_][Q_] += t * apq;
  A[P_][Q_] = 0.0; A[Q_][P_] = 0.0;
  A[R_][P_] = c * arp - s * arq; A[P_][R_] = A[R_][P_];
  A[R_][Q_] = s * arp + c * arq; A[Q_][R_] = A[R_][Q_];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double vp = V[i][P_], vq = V[i][Q_];
    V[i][P_] = c * vp - s * vq;
    V[i][Q_] = s * vp + c * vq;
  }
}

// unit eigenvector of the smallest eigenvalue of the symmetric matrix (xx, xy, xz, yy, yz, zz): cyclic Jacobi, which resolves an
// eigenvector to a few ulp of |C| / gap whatever the spread of the eigenvalues
__device__ inline void smallest_eigenvector(const double* c6, double* nv) {
  double A[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < 12; ++sweep) {
    if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
    jacobi_rotate<0, 1>(A, V);
    jacobi_rotate<0, 2>(A, V);
    jacobi_rotate<1, 2>(A, V);
  }
  const bool m1 = A[1][1] < A[0][0];
  const double l01 = m1 ? A[1][1] : A[0][0];
  const bool m2 = A[2][2] < l01;
#pragma unroll
  for (int i = 0; i < 3; ++i) nv[i] = m2 ? V[i][2] : (m1 ? V[i][1] : V[i][0]);
  const double nn = sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
  nv[0] /= nn; nv[1] /= nn; nv[2] /= nn;
}

__global__ __launch_bounds__(64) void plane_refit_kernel(PrParams q) {
  const int p = blockIdx.x, lane = threadIdx.x;
  PrHdr* h = q.hdr + p;
  if (h->status != 0) return;
  const int nseg = (h->count + PR_SEG - 1) / PR_SEG;
  double c6[6];
  pr_merge_segments<6>(q.pc + (long long)p * q.nseg * 6, nseg, lane, c6);
  if (lane != 0) return;
  double nv[3], d;
  smallest_eigenvector(c6, nv);
  if (nv[1] > 0.0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
  d = -((nv[0] * h->mu[0] + nv[1] * h->mu[1]) + nv[2] * h->mu[2]);
  if (!(finite_f64(nv[0]) && finite_f64(nv[1]) && finite_f64(nv[2]) && finite_f64(d))) {   // the trial's own plane
    const double rs = sqrt(h->s);
    nv[0] = h->w[0] / rs; nv[1] = h->w[1] / rs; nv[2] = h->w[2] / rs;
    if (nv[1] > 0.0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
    d = -((nv[0] * h->a[0] + nv[1] * h->a[1]) + nv[2] * h->a[2]);
  }
  h->plane[0] = nv[0]; h->plane[1] = nv[1]; h->plane[2] = nv[2]; h->plane[3] = d;
  double* o = q.plane + (long long)p * 4;
  o[0] = nv[0]; o[1] = nv[1]; o[2] = nv[2]; o[3] = d;
}

// ---- recount, report ------------------------------------------------------------------------------------------------------------
// r = n_x x + n_y y + n_z z + d under the reported plane; final inlier iff |r| <= tol.  The grid covers the rows' capacity: every slot of
// `inliers` gets its flag, 0 behind a frame's count and for a frame that was not fitted.
__global__ __launch_bounds__(PR_NT) void plane_recount_kernel(PrParams q) {
  __shared__ double red[PR_ROWS];
  __shared__ int redk[PR_ROWS];
  const int seg = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PrHdr* h = q.hdr + p;
  const bool fitted = h->status == 0;
  const int n = fitted ? h->count : 0;
  const bool live = (long long)seg * PR_SEG < (long long)n;   // uniform
  if (!live && !q.inliers) return;
  const double nx = h->plane[0], ny = h->plane[1], nz = h->plane[2], d = h->plane[3];
  const double* pts = q.pts + (long long)p * q.stride * 3;
  double v[1] = {0.0};
  int k = 0;
#pragma unroll
  for (int j = 0; j < PR_PER; ++j) {
    const long long i = (long long)seg * PR_SEG + j * PR_NT + tid;
    bool in = false;
    double r = 0.0;
    if (live) {
      const PrSample sm = pr_sample(pts, (int)i, n, q.thr_abs, q.thr_rel);
      r = ((nx * sm.x + ny * sm.y) + nz * sm.z) + d;
      in = fabs(r) <= sm.tol;
    }
    v[0] += in ? r * r : 0.0;
    k += in ? 1 : 0;
    if (q.inliers && i < q.stride) q.inliers[(long long)p * q.stride + i] = in ? 1 : 0;
  }
  if (!live) return;
  k = wave_sum_i(k);
  if (lane == 0) redk[wave] = k;
  pr_block_sum<1>(v, red, tid);
  if (tid == 0) {
    q.prr[(long long)p * q.nseg + seg] = v[0];
    q.prk[(long long)p * q.nseg + seg] = (redk[0] + redk[1]) + (redk[2] + redk[3]);
  }
}

__global__ __launch_bounds__(64) void plane_report_kernel(PrParams q) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const PrHdr* h = q.hdr + p;
  if (h->status != 0) return;
  const int nseg = (h->count + PR_SEG - 1) / PR_SEG;
  double v[1];
  pr_merge_segments<1>(q.prr + (long long)p * q.nseg, nseg, lane, v);
  int k = 0;
  for (int r = lane; r < nseg; r += 64) k += q.prk[(long long)p * q.nseg + r];
  k = wave_sum_i(k);
  if (lane == 0) {
    q.n_inliers[p] = k;
    q.rms[p] = k > 0 ? sqrt(v[0] / (double)k) : NAN;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }
inline bool finite_host(double v) { return v - v == 0.0; }

struct PsGrid { long long gh, gw, cap, nchunk; };
inline PsGrid ps_grid(long long H, long long W, long long step) {
  PsGrid g;
  g.gh = (H + step - 1) / step; g.gw = (W + step - 1) / step;
  g.cap = g.gh * g.gw;
  g.nchunk = g.cap > 0 ? (g.cap + PS_CHUNK - 1) / PS_CHUNK : 1;
  return g;
}

const char* ps_check(const la3d_plane_select_args* a, int* rc) {
  *rc = LA3D_ERR_ARG;
  if (!a) return "NULL argument block";
  if (a->struct_size != (int32_t)sizeof(la3d_plane_select_args)) return "struct_size is not sizeof(la3d_plane_select_args)";
  if (a->P < 0 || a->H < 0 || a->W < 0) return "negative P, H or W";
  if (a->step < 1) return "step must be at least 1";
  if (a->near_depth != a->near_depth || a->far_depth != a->far_depth) return "near_depth or far_depth is NaN";
  if (a->k_stride != 0 && a->k_stride < 9) return "k_stride must be 0 (shared) or >= 9";
  if (a->reserved != 0) return "reserved must be 0";
  if (a->candidates && (a->cand_width < a->W || (a->cand_width & 31) || a->cand_plane_stride < 0))
    return "candidates need a stored width that is a multiple of 32 and >= W, and a plane stride >= 0";
  if ((addr(a->depth) | addr(a->candidates) | addr(a->pixel) | addr(a->workspace)) & 3u) return "a pointer is not 4-byte aligned";
  if ((addr(a->K) | addr(a->points) | addr(a->counts)) & 7u) return "K, points and counts must be 8-byte aligned";
  if (a->candidates && a->cand_plane_stride != 0 && a->cand_plane_stride < (long long)a->H * a->cand_width / 32)
    return "cand_plane_stride below the words of a plane";
  const PsGrid g = ps_grid(a->H, a->W, a->step);
  if (a->P > 0 && (!a->counts || !a->workspace || (g.cap > 0 && (!a->depth || !a->K || !a->points || !a->pixel))))
    return "NULL pointer with work to do";
  *rc = LA3D_ERR_UNSUPPORTED;
  if ((long long)a->H * a->W > 0x40000000LL) return "H * W > 2^30: pixel and grid indices are int32";
  if (a->P > 65535) return "more than 65535 images";
  *rc = LA3D_SUCCESS;
  return nullptr;
}

const char* pr_check(const la3d_plane_ransac_args* a, int* rc) {
  *rc = LA3D_ERR_ARG;
  if (!a) return "NULL argument block";
  if (a->struct_size != (int32_t)sizeof(la3d_plane_ransac_args)) return "struct_size is not sizeof(la3d_plane_ransac_args)";
  if (a->P < 0 || a->n < 0) return "negative P or n";
  if (a->max_trials < 1) return "max_trials must be at least 1";
  if (!(a->thr_abs >= 0.0) || !(a->thr_rel >= 0.0) || (a->thr_abs == 0.0 && a->thr_rel == 0.0) || !finite_host(a->thr_abs) || !finite_host(a->thr_rel))
    return "thr_abs and thr_rel must be finite and >= 0, and not both zero";
  if (!(a->cos2_tilt >= 0.0 && a->cos2_tilt <= 1.0)) return "cos2_tilt outside [0, 1]";
  if (a->min_inliers < 0) return "min_inliers must be >= 0 (0: the default, 3)";
  if ((addr(a->subsets) | addr(a->k_trial) | addr(a->n_inliers) | addr(a->best_trial) | addr(a->status)) & 3u)
    return "a pointer is not 4-byte aligned";
  if ((addr(a->points) | addr(a->counts) | addr(a->plane) | addr(a->rms)) & 7u) return "points, counts, plane and rms must be 8-byte aligned";
  if (addr(a->workspace) & 15u) return "the workspace must be 16-byte aligned";
  if (a->P > 0 && (!a->counts || !a->plane || !a->k_trial || !a->n_inliers || !a->best_trial || !a->rms || !a->status || !a->workspace ||
                   (a->n > 0 && !a->points)))
    return "NULL pointer with work to do";
  *rc = LA3D_ERR_UNSUPPORTED;
  if (a->n > LA3D_PLANE_MAX_N) return "more than LA3D_PLANE_MAX_N samples per frame";
  if (a->max_trials > LA3D_PLANE_MAX_TRIALS) return "more than LA3D_PLANE_MAX_TRIALS trials";
  if (a->P > 65535) return "more than 65535 frames";
  *rc = LA3D_SUCCESS;
  return nullptr;
}

}  // namespace

extern "C" {

size_t la3d_plane_select_workspace_bytes(int P, int H, int W, int step) {
  if (P <= 0 || H < 0 || W < 0 || step < 1) return 16;
  return (size_t)P * (size_t)ps_grid(H, W, step).nchunk * sizeof(int32_t);
}

int la3d_plane_select_batch(const la3d_plane_select_args* a) {
  int rc;
  if (const char* what = ps_check(a, &rc)) return refuse("la3d_plane_select_batch", what, rc);
  if (a->P == 0) return LA3D_SUCCESS;
  const PsGrid g = ps_grid(a->H, a->W, a->step);
  PsParams q;
  q.P = a->P; q.H = a->H; q.W = a->W; q.step = a->step; q.gw = (int)(g.gw > 0 ? g.gw : 1); q.cap = (int)g.cap; q.nchunk = (int)g.nchunk;
  q.k_stride = a->k_stride;
  q.near_d = a->near_depth; q.far_d = a->far_depth;
  q.depth = a->depth; q.K = a->K;
  q.cand = a->candidates;
  q.cand_width = a->cand_width;
  q.cand_stride = a->cand_plane_stride ? a->cand_plane_stride : (long long)a->H * a->cand_width / 32;
  q.points = a->points; q.pixel = a->pixel; q.counts = reinterpret_cast<long long*>(a->counts);
  q.ws = static_cast<int*>(a->workspace);
  hipStream_t s = static_cast<hipStream_t>(a->stream);
  const dim3 grid((unsigned)g.nchunk, (unsigned)a->P);
  hipLaunchKernelGGL(plane_select_count_kernel, grid, dim3(PS_NT), 0, s, q);
  hipLaunchKernelGGL(plane_select_write_kernel, grid, dim3(PS_NT), 0, s, q);
  return check_launch("la3d_plane_select_batch");
}

size_t la3d_plane_ransac_workspace_bytes(int P, int64_t n, int max_trials) {
  if (P <= 0 || n < 0 || max_trials < 1 || n > LA3D_PLANE_MAX_N || max_trials > LA3D_PLANE_MAX_TRIALS) return 16;
  return pr_layout(P, n, max_trials).total;
}

int la3d_plane_ransac_batch(const la3d_plane_ransac_args* a) {
  int rc;
  if (const char* what = pr_check(a, &rc)) return refuse("la3d_plane_ransac_batch", what, rc);
  if (a->P == 0) return LA3D_SUCCESS;
  const int P = a->P, T = a->max_trials;
  const PrLayout L = pr_layout(P, a->n, T);
  unsigned char* ws = static_cast<unsigned char*>(a->workspace);
  PrParams q;
  q.pts = a->points; q.counts = reinterpret_cast<const long long*>(a->counts);
  q.stride = a->n;
  q.thr_abs = a->thr_abs; q.thr_rel = a->thr_rel; q.cos2_tilt = a->cos2_tilt;
  q.T = T; q.min_inliers = a->min_inliers > 0 ? a->min_inliers : 3;
  q.subsets = a->subsets; q.seed = a->seed;
  q.plane = a->plane; q.k_trial = a->k_trial; q.n_inliers = a->n_inliers; q.best_trial = a->best_trial; q.status = a->status;
  q.rms = a->rms; q.inliers = a->inliers;
  q.hdr = reinterpret_cast<PrHdr*>(ws + L.hdr);
  q.trials = reinterpret_cast<double*>(ws + L.trials);
  q.pk = reinterpret_cast<int*>(ws + L.pk);
  q.pm = reinterpret_cast<double*>(ws + L.pm); q.pc = reinterpret_cast<double*>(ws + L.pc); q.prr = reinterpret_cast<double*>(ws + L.prr);
  q.prk = reinterpret_cast<int*>(ws + L.prk);
  q.nseg = L.nseg;
  hipStream_t s = static_cast<hipStream_t>(a->stream);
  const dim3 segs((unsigned)L.nseg, (unsigned)P);
  hipLaunchKernelGGL(plane_trials_kernel, dim3((unsigned)((T + PR_NT - 1) / PR_NT), (unsigned)P), dim3(PR_NT), 0, s, q);
  const size_t cand_lds = (size_t)T * (PR_TL * 8 + PR_ROWS * 4);   // at most 72 KiB (T = 1024)
  allow_big_lds(reinterpret_cast<const void*>(plane_candidates_kernel));
  hipLaunchKernelGGL(plane_candidates_kernel, segs, dim3(PR_NT), cand_lds, s, q);
  hipLaunchKernelGGL(plane_pick_kernel, dim3((unsigned)P), dim3(PR_NT), 0, s, q);
  hipLaunchKernelGGL(plane_moments_kernel<false>, segs, dim3(PR_NT), 0, s, q);
  hipLaunchKernelGGL(plane_centre_kernel, dim3((unsigned)P), dim3(64), 0, s, q);
  hipLaunchKernelGGL(plane_moments_kernel<true>, segs, dim3(PR_NT), 0, s, q);
  hipLaunchKernelGGL(plane_refit_kernel, dim3((unsigned)P), dim3(64), 0, s, q);
  hipLaunchKernelGGL(plane_recount_kernel, segs, dim3(PR_NT), 0, s, q);
  hipLaunchKernelGGL(plane_report_kernel, dim3((unsigned)P), dim3(64), 0, s, q);
  return check_launch("la3d_plane_ransac_batch");
}

}  // extern "C"
