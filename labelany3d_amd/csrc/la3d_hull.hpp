// la3d_hull.hpp - the convex-hull yaw (reference src/util_3dbox.py:189-224) shared by the point-cloud kernels (la3d_points.hip) and
// the hull finish of the instance engine (la3d_instance.hip): the LDS layout, Andrew's monotone chain and the minimum-area
// rectangle over the hull edges.  Workgroups of NTP threads; `Sh` is the caller's shared struct with int fields nvalid (points
// held in hs->x / hs->z) and hull_n (out: hull vertices).
#pragma once
#include "la3d_device.hpp"

using namespace la3d;

namespace {
constexpr int HULL_MAX = 2048;  // points the convex-hull method holds in LDS (the reference feeds it <= 500, :123; round 6: 512 -> 2048,
                                // 24 bytes of LDS per point: coordinates, candidate list, survivor flags, chain stacks)
constexpr int HULL_SMALL = 512; // ... and the form for calls that promise at most 512 valid rows per cloud (LA3D_HINT_HULL_512, a sample_idx
                                // array, the scalar drop-in's <= 500 points): 12 KB of LDS instead of 48 - eight workgroups per CU instead
                                // of three (the chain is one lane's serial work: 7.4 M vs 5.7 M clouds/s on 500-point batches)

// LDS of the convex-hull method (separate struct: only the hull instantiation pays for it)
template <int HCAP>
struct alignas(16) SharedHullT {
  double x[HCAP], z[HCAP];              // valid (x', z') footprint, sorted lexicographically
  unsigned short cand[HCAP];            // current candidates of the chain, in sorted order
  unsigned short flag[HCAP];            // survivor flags by point
  unsigned short hull[2 * HCAP + 2];
  double best_area[NTP / 64], best_yaw[NTP / 64];   // per wave: the first strict minimum among its edges ...
  int best_edge[NTP / 64];                          // ... and that edge's index (ties across waves go to the smaller index)
};

// One pass of Andrew's monotone chain: visits cnt entries of the candidate list cl starting at position q0 in direction dq, pushes
// point indices on the stack S (k0 entries on entry; a pop needs at least t), returns the stack size.  The coordinates of the two
// stack tops are carried in registers, so a step that pops nothing waits for no dependent LDS read.  The turn test is the textbook
// cross(o, a, b) = (xa - xo)(zb - zo) - (za - zo)(xb - xo) <= 0 -> pop.
template <typename SharedHull>
__device__ inline int chain_pass(const SharedHull* hs, const unsigned short* cl, int q0, int dq, int cnt, unsigned short* S, int k0, int t) {
  int k = k0;
  double ox = 0, oz = 0, ax = 0, az = 0;
  if (k >= 1) { const int a = S[k - 1]; ax = hs->x[a]; az = hs->z[a]; }
  if (k >= 2) { const int o = S[k - 2]; ox = hs->x[o]; oz = hs->z[o]; }
  for (int c = 0, q = q0; c < cnt; ++c, q += dq) {
    const int i = cl[q];
    const double px = hs->x[i], pz = hs->z[i];
    while (k >= t) {
      // both products ROUNDED (no contraction into an fma, which keeps one product exact: for a point that repeats the stack top -
      // the reference's subsample draws with replacement, src/util_3dbox.py:124 - the two products are the same two factors and
      // the difference must be exactly zero, so that the repeat is popped; fused, the difference was the rounding error of one
      // product, of either sign, and a repeated hull vertex could stay: a zero-length edge, i.e. a candidate yaw of 0 the
      // reference never tries.  Found by profiles/r06/fuzz_points.py (round 6): every batched call with sample_idx and
      // method = convex_hull was exposed, the scalar drop-in too)
      double cr;
      {
#pragma clang fp contract(off)
        const double t0 = (ax - ox) * (pz - oz), t1 = (az - oz) * (px - ox);
        cr = t0 - t1;
      }
      if (!(cr <= 0)) break;
      --k;
      ax = ox; az = oz;
      if (k >= 2) { const int o = S[k - 2]; ox = hs->x[o]; oz = hs->z[o]; }
    }
    S[k++] = (unsigned short)i;
    ox = ax; oz = az; ax = px; az = pz;
  }
  return k;
}

// Minimum-area enclosing rectangle over hull-edge directions — reference src/util_3dbox.py:189-224
// (SciPy/Qhull there; here: bitonic sort in LDS, Andrew's monotone chain, one thread per hull edge).
// Reproduces the reference's conventions: yaw = atan2(edge_z, edge_x); points rotated by
// [[cos,-sin],[sin,cos]] (:204-208); area of the axis-aligned extent; the FIRST strict minimum wins
// (:216) in counter-clockwise vertex order.  Returns false when there is no 2-D hull (fewer than 3
// vertices: Qhull raises there and the reference falls back to PCA, :222-224).
template <typename SharedHull, typename Sh>
__device__ inline bool hull_yaw(SharedHull* hs, Sh* sh, int tid, double* yaw_out) {
  const int n = sh->nvalid;
  // pad to a power of two for the bitonic network: the smallest one that holds the cloud (512 for the reference's 500 points)
  int P2 = 64;
  while (P2 < n) P2 <<= 1;                                             // uniform; n <= HULL_MAX
  for (int i = n + tid; i < P2; i += NTP) { hs->x[i] = INFINITY; hs->z[i] = INFINITY; }
  __syncthreads();
  for (int k = 2; k <= P2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P2; i += NTP) {
        const int l = i ^ j;
        if (l > i) {
          const double xi = hs->x[i], zi = hs->z[i], xl = hs->x[l], zl = hs->z[l];
          const bool gt = (xi > xl) || (xi == xl && zi > zl);
          if (((i & k) == 0) ? gt : !gt) { hs->x[i] = xl; hs->z[i] = zl; hs->x[l] = xi; hs->z[l] = zi; }
        }
      }
      __syncthreads();
    }
  // Andrew's monotone chain is serial (every step depends on the stack the previous one left) and each of its cross products is a
  // chain of dependent LDS reads - one lane needed ~150 us for 500 points.  Round 3: (1) sixteen lanes each run the chain over a
  // sixteenth of the sorted points and mark what survives in their chunk (a point inside its chunk's hull cannot be a vertex of the
  // whole hull; collinear points drop out either way), the survivors are compacted in sorted order; (2) four lanes do the same
  // over quarters of the survivors; (3) one lane runs the SAME chain over what is left.  With exact orientation predicates the
  // vertex sequence - hence every edge, area and the winning yaw - is the one the chain over all points gives; the fp64 cross
  // products are rounded, so in NEARLY collinear configurations (or with duplicate points straddling a chunk boundary) a point
  // may be kept by one form and dropped by the other: the hulls then differ by a vertex that moves no edge beyond rounding, and the
  // minimum-area yaw can only move between edges whose areas tie to rounding (the documented don't-care; profiles/r03/stress_hull.py
  // holds both forms to the oracle with a yaw / area tolerance).  The two stack tops live in registers (chain_pass).
  unsigned short* cl = hs->cand;   // current candidates in sorted order
  for (int i = tid; i < n; i += NTP) cl[i] = (unsigned short)i;
  int m = n;
  for (int level = 0; level < 2; ++level) {
    const int nch = level == 0 ? 16 : 4;
    if (m <= 4 * nch) continue;                                      // uniform
    for (int i = tid; i < n; i += NTP) hs->flag[i] = 0;              // survivor flags by point
    __syncthreads();
    if (tid < nch) {
      const int lo = (int)((long long)m * tid / nch), hi = (int)((long long)m * (tid + 1) / nch);
      unsigned short* S = hs->hull + lo;                             // this lane's stack: as many slots as its chunk has entries
      for (int pass = 0; pass < 2; ++pass) {                         // lower hull left -> right, then upper hull right -> left
        const int k = chain_pass(hs, cl, pass == 0 ? lo : hi - 1, pass == 0 ? 1 : -1, hi - lo, S, 0, 2);
        for (int q = 0; q < k; ++q) hs->flag[S[q]] = 1;
      }
    }
    __syncthreads();
    if (tid < 64) {                                                  // in-place compaction of the survivors, ascending (one wave:
      int base = 0;                                                  // a block's reads precede its writes, and it writes behind itself)
      for (int i0 = 0; i0 < m; i0 += 64) {
        const int i = i0 + tid;
        const unsigned short id = i < m ? cl[i] : (unsigned short)0;
        const bool on = i < m && hs->flag[id] != 0;
        const unsigned long long bal = __ballot(on);
        if (on) cl[base + __popcll(bal & ((1ull << tid) - 1ull))] = id;
        base += __popcll(bal);
      }
      if (tid == 0) sh->hull_n = base;                               // (number of survivors, until the chain below replaces it)
    }
    __syncthreads();
    m = sh->hull_n;
    __syncthreads();
  }
  if (tid == 0) {  // monotone chain over the survivors: lower hull left->right, then upper hull right->left (counter-clockwise)
    unsigned short* H = hs->hull;
    int k = chain_pass(hs, cl, 0, 1, m, H, 0, 2);
    k = chain_pass(hs, cl, m - 2, -1, m - 1, H, k, k + 1);
    sh->hull_n = k - 1;  // last vertex repeats the first
  }
  __syncthreads();
  const int h = sh->hull_n;
  if (h < 3) return false;
  // one hull edge per wave at a time, lanes over the points (min / max are order independent: the areas are those of a serial sweep);
  // every wave keeps the FIRST strict minimum among its edges (e = wave, wave + 8, ... ascending), thread 0 then takes the smallest
  // area over the waves, ties to the smaller edge index: the first strict minimum of the serial sweep (:216), with no per-edge array
  const int lane = tid & 63, wave = tid >> 6;
  double wbest = INFINITY, wyaw = 0.0;
  int wedge = 0x7fffffff;
  for (int e = wave; e < h; e += NTP / 64) {
    const int i0 = hs->hull[e], i1 = hs->hull[(e + 1 == h) ? 0 : e + 1];
    const double yaw = atan2(hs->z[i1] - hs->z[i0], hs->x[i1] - hs->x[i0]);
    const double cs = cos(yaw), sn = sin(yaw);
    double xlo = INFINITY, xhi = -INFINITY, zlo = INFINITY, zhi = -INFINITY;
    for (int j = lane; j < n; j += 64) {
      const double px = hs->x[j], pz = hs->z[j];
      const double rx = cs * px - sn * pz, rz = sn * px + cs * pz;
      xlo = fmin(xlo, rx); xhi = fmax(xhi, rx); zlo = fmin(zlo, rz); zhi = fmax(zhi, rz);
    }
    xlo = wave_min(xlo); xhi = wave_max(xhi); zlo = wave_min(zlo); zhi = wave_max(zhi);
    const double area = (xhi - xlo) * (zhi - zlo);
    if (area < wbest) { wbest = area; wyaw = yaw; wedge = e; }   // (every lane holds the wave's values)
  }
  if (lane == 0) { hs->best_area[wave] = wbest; hs->best_yaw[wave] = wyaw; hs->best_edge[wave] = wedge; }
  __syncthreads();
  if (tid == 0) {
    double best = INFINITY, by = 0.0;
    int be = 0x7fffffff;
    for (int w = 0; w < NTP / 64; ++w) {
      const double a = hs->best_area[w];
      if (a < best || (a == best && hs->best_edge[w] < be)) { best = a; by = hs->best_yaw[w]; be = hs->best_edge[w]; }
    }
    hs->best_yaw[0] = by;
  }
  __syncthreads();
  *yaw_out = hs->best_yaw[0];
  return true;
}

// ------------------------------------------------------------------------------------------
// Hand-off of a convex-hull call of la3d_fit_instances_ex (la3d_instance.hip): the hull instantiation of the fit kernel leaves, per
// instance, a header of HH_D doubles and a payload in the workspace; hull_finish_kernel (one workgroup per instance) reads them.
//   full-mask mode:  payload = the per-column depth ranges of the single pass, colmin[W] | colmax[W] as sign-flip keys (hull_key)
//   subsample mode:  payload = HULL_SMALL points (x', y', z') in the ground-aligned frame, NaN where a thread holds none
// HH_STATE: 0 = finish this instance; anything else = the fit kernel has written the instance's final status and NaN record itself
// (filtered, rejected, refused).
// ------------------------------------------------------------------------------------------
constexpr int HH_D = 32;
constexpr int HH_STATE = 0, HH_NVALID = 1, HH_NM = 2, HH_CYAW = 3, HH_SYAW = 4, HH_GAP = 5, HH_YLO = 6, HH_YHI = 7, HH_RG = 8,
              HH_A00 = 17, HH_A02 = 18, HH_NPTS = 19;
__host__ __device__ inline size_t hull_stride_bytes(bool sample, int W) {
  return (size_t)HH_D * 8 + (sample ? (size_t)HULL_SMALL * 24 : (size_t)((2 * W + 3) & ~3) * 4);
}
__device__ inline double* hull_slot(double* area, int inst, size_t stride) {
  return reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(area) + (size_t)inst * stride);
}
// float bit pattern -> unsigned key that orders like the float, negative values included (NaN never gets here)
__device__ inline unsigned hull_key(unsigned b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ inline float hull_unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

}  // namespace
