// la3d_point.hpp - one back-projected pixel, shared by the units whose rows must equal la3d_unproject_batch's bit for bit: the
// instance point clouds (la3d_cloud.hip) and the sample select of the ground plane (la3d_plane.hip).
#pragma once
#include "la3d_device.hpp"

namespace la3d {

// (d * Kinv) @ [u, v, 1], then the identity R, t multiply: unproject_frame of la3d_masks.hip, term for term (src/util.py:71-74) - a
// NaN / inf depth poisons its row exactly as there
__device__ inline void cloud_point(double d, unsigned u, unsigned v, const double* kinv, double* w) {
  const double ud = (double)u, vd = (double)v;
  double q[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) q[r] = (d * kinv[r * 3]) * ud + (d * kinv[r * 3 + 1]) * vd + (d * kinv[r * 3 + 2]);
  w[0] = 1.0 * q[0] + 0.0 * q[1] + 0.0 * q[2] + 0.0;
  w[1] = 0.0 * q[0] + 1.0 * q[1] + 0.0 * q[2] + 0.0;
  w[2] = 0.0 * q[0] + 0.0 * q[1] + 1.0 * q[2] + 0.0;
}

}  // namespace la3d
