// la3d_hull_finish.hip - the kernels BEHIND the fit kernel of a convex-hull call and their launches.  They
// read no depth, so they exist once: the instance engine's three units (la3d_instance.hip for float32, float16 and uint16 planes)
// launch them through hull_finish_launch / hull_refuse_launch (la3d_engines.hpp).
#include <cstddef>

#include "la3d_device.hpp"
#include "la3d_engines.hpp"
#include "la3d_hull.hpp"

namespace {
// ------------------------------------------------------------------------------------------
// hull finish: one workgroup of NTP threads per instance - candidates -> hull_yaw -> extents over the candidates under the hull yaw
// (the extents of a point set along ANY direction are taken at hull vertices, and every hull vertex is a candidate) -> record.
// ------------------------------------------------------------------------------------------
struct alignas(16) SharedF {
  double part[NWAVEP][8];
  double cyaw, syaw;
  int nvalid;       // candidates held in hs.x / hs.z (hull_yaw's point count)
  int hull_n;
  int fill;
};

template <bool SAMPLE, int HCAP>
__global__ __launch_bounds__(NTP) void hull_finish_kernel(const FitParams p, unsigned long long stride) {
  __shared__ SharedF sh;
  __shared__ SharedHullT<HCAP> hs;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int inst = blockIdx.x;
  const double* hh = hull_slot(p.geo, inst, (size_t)stride);
  if (hh[HH_STATE] != 0.0) return;   // uniform: the fit kernel has finished this instance itself
  if (tid == 0) { sh.fill = 0; sh.hull_n = 0; }
  __syncthreads();
  double ylo = INFINITY, yhi = -INFINITY;
  if (SAMPLE) {
    const int npts = min((int)hh[HH_NPTS], HULL_SMALL);
    const double* pts = hh + HH_D;
    for (int i = tid; i < npts; i += NTP) {
      const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
      if (x == x) {   // (a point the fit kernel dropped is three NaNs)
        const int slot = atomicAdd(&sh.fill, 1);
        if (slot < HCAP) { hs.x[slot] = x; hs.z[slot] = z; }
        ylo = fmin(ylo, y); yhi = fmax(yhi, y);
      }
    }
  } else {
    const unsigned* col = reinterpret_cast<const unsigned*>(hh + HH_D);
    const double a00 = hh[HH_A00], a02 = hh[HH_A02];
    if (tid == 0) { ylo = hh[HH_YLO]; yhi = hh[HH_YHI]; }
    for (int u = tid; u < p.W; u += NTP) {
      const unsigned lo = col[u], hi = col[p.W + u];
      if (lo <= hi) {   // the column holds a valid pixel: the two ends of its ray (one point when they coincide)
        const int k = lo == hi ? 1 : 2;
        const int slot = atomicAdd(&sh.fill, k);
        if (slot + k <= HCAP) {
          const double r0 = fma(a00, (double)u, a02), dlo = (double)hull_unkey(lo), dhi = (double)hull_unkey(hi);
          hs.x[slot] = dlo * r0; hs.z[slot] = dlo;
          if (k == 2) { hs.x[slot + 1] = dhi * r0; hs.z[slot + 1] = dhi; }
        }
      }
    }
  }
  __syncthreads();
  const int n = sh.fill;
  double* out = p.out + (long long)inst * LA3D_REC;
  double* aux = p.aux ? p.aux + (long long)inst * LA3D_AUX : nullptr;
  if (n > HCAP) {   // uniform: more than HCAP candidates (one per column whose two ends coincide, two otherwise) - refused, never fitted as PCA
    if (tid == 0) write_no_box(p, inst, LA3D_BOX_UNSUPPORTED, hh[HH_NVALID], hh[HH_NM]);
    return;
  }
  if (tid == 0) { sh.nvalid = n; sh.cyaw = hh[HH_CYAW]; sh.syaw = hh[HH_SYAW]; }
  __syncthreads();
  double yaw = 0.0;
  const bool by_hull = hull_yaw(&hs, &sh, tid, &yaw);   // false: fewer than 3 hull vertices - the PCA axis stands (reference :222-224)
  if (by_hull && tid == 0) {
    double s_, c_;
    sincos(yaw, &s_, &c_);
    sh.cyaw = c_; sh.syaw = s_;
  }
  __syncthreads();
  const double cy = sh.cyaw, sy = sh.syaw;
  double xlo = INFINITY, xhi = -INFINITY, zlo = INFINITY, zhi = -INFINITY;
  for (int i = tid; i < n; i += NTP) {
    const double x = hs.x[i], z = hs.z[i];
    const double x2 = cy * x + sy * z, z2 = -sy * x + cy * z;   // rotate_y(yaw) @ rotated^T  (:154)
    xlo = fmin(xlo, x2); xhi = fmax(xhi, x2); zlo = fmin(zlo, z2); zhi = fmax(zhi, z2);
  }
  {
    const double r0 = wave_min(xlo), r1 = wave_max(xhi), r2 = wave_min(zlo), r3 = wave_max(zhi), r4 = wave_min(ylo), r5 = wave_max(yhi);
    if (lane == 0) { double* pp = sh.part[wave]; pp[0] = r0; pp[1] = r1; pp[2] = r2; pp[3] = r3; pp[4] = r4; pp[5] = r5; }
  }
  __syncthreads();
  if (wave == 0) {
    double xmin = INFINITY, xmax = -INFINITY, zmin = INFINITY, zmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int w = 0; w < NWAVEP; ++w) {
      xmin = fmin(xmin, sh.part[w][0]); xmax = fmax(xmax, sh.part[w][1]); zmin = fmin(zmin, sh.part[w][2]); zmax = fmax(zmax, sh.part[w][3]);
      ymin = fmin(ymin, sh.part[w][4]); ymax = fmax(ymax, sh.part[w][5]);
    }
    double Rg[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rg[i] = hh[HH_RG + i];
    if (p.proj) {   // uniform
      const int img = p.image_index ? p.image_index[inst] : inst;
      write_box_wave(out, Rg, cy, sy, xmin, xmax, ymin, ymax, zmin, zmax, lane, p.proj + (long long)inst * 8, p.K + (long long)img * p.k_stride,
                     p.proj_w, p.proj_h);
    } else {
      write_box_wave(out, Rg, cy, sy, xmin, xmax, ymin, ymax, zmin, zmax, lane);
    }
  } else if (tid == 64) {
    if (aux) {
      aux[0] = by_hull ? yaw : atan2(sy, cy); aux[1] = hh[HH_NVALID]; aux[2] = hh[HH_NM];
      aux[3] = by_hull ? -(double)sh.hull_n : hh[HH_GAP];   // negative: the hull decided the yaw (value = number of hull vertices)
    }
    p.status[inst] = LA3D_BOX_OK;
  }
}

// a hull call in full-mask mode on a frame outside the tiled vector path: every instance is refused (status 5, NaN record)
__global__ __launch_bounds__(256) void hull_refuse_kernel(const FitParams p) {
  const int inst = blockIdx.x * 256 + threadIdx.x;
  if (inst < p.B) write_no_box(p, inst, LA3D_BOX_UNSUPPORTED, 0.0, NAN);
}
}  // namespace

namespace la3d {
int hull_finish_launch(const FitParams& p, bool sample, hipStream_t s) {
  const unsigned long long stride = hull_stride_bytes(sample, p.W);
  if (sample) hipLaunchKernelGGL((hull_finish_kernel<true, HULL_SMALL>), dim3(p.B), dim3(NTP), 0, s, p, stride);
  else hipLaunchKernelGGL((hull_finish_kernel<false, HULL_MAX>), dim3(p.B), dim3(NTP), 0, s, p, stride);
  return check_launch("hull_finish_kernel");
}
int hull_refuse_launch(const FitParams& p, hipStream_t s) {
  hipLaunchKernelGGL(hull_refuse_kernel, dim3((p.B + 255) / 256), dim3(256), 0, s, p);
  return check_launch("hull_refuse_kernel");
}
}  // namespace la3d
