// la3d_depth16.hip - the packers of the 16-bit depth planes (include/la3d.h "16-bit depth planes"): float32 planes -> IEEE float16 or
// uint16 x scale planes and back.  Streaming kernels in the style of la3d_pack_mask_bits: any plane stride and any (element) alignment
// of either side; a 16-byte store form stands in front of the general one.  The value rule of unpacking is depth_bits
// (la3d_device.hpp) - the one the fit kernels apply.
#include <cstdint>

#include "la3d_device.hpp"

using namespace la3d;

namespace {
// float32 -> the stored 16-bit word
template <int DTYPE>
__device__ inline unsigned pack16(float d, float scale) {
  if (DTYPE == LA3D_DTYPE_F16) {   // round to nearest even, overflow to inf, subnormals kept: astype(np.float16)
    return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)d);
  } else {                          // q = rint(d / scale) in float32; NaN, +-inf and d <= 0 -> 0; q > 65535 -> 65535
    if (!(d > 0.0f) || !finite_f32(d)) return 0u;
    const float q = rintf(d / scale);
    return q > 65535.0f ? 65535u : (unsigned)q;
  }
}

// one thread per group of 8 output pixels of a padded row (W_out); vec: the group is one 16-byte store
template <int DTYPE>
__global__ __launch_bounds__(256) void pack_depth16_kernel(const float* __restrict__ depth, long long plane_stride, int P, int H, int W,
                                                           int W_out, float scale, unsigned short* __restrict__ out,
                                                           long long out_plane_stride, int vec) {
  const int gpr = (W_out + 7) >> 3;   // groups per row
  const long long total = (long long)P * H * gpr;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
    const long long row = g / gpr;
    const int c0 = (int)(g - row * gpr) * 8;
    const long long pl = row / H;
    const int r = (int)(row - pl * H);
    const float* s = depth + pl * plane_stride + (long long)r * W;
    unsigned short* o = out + pl * out_plane_stride + (long long)r * W_out + c0;
    unsigned w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = (c0 + k < W) ? pack16<DTYPE>(s[c0 + k], scale) : 0u;   // columns [W, W_out): zeros
    if (vec) {   // uniform: W_out % 8 == 0, base and plane stride 16-byte aligned
      u32x4 v;
      v.x = w[0] | (w[1] << 16); v.y = w[2] | (w[3] << 16); v.z = w[4] | (w[5] << 16); v.w = w[6] | (w[7] << 16);
      *reinterpret_cast<u32x4*>(o) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (c0 + k < W_out) o[k] = (unsigned short)w[k];
    }
  }
}

// one thread per output pixel: the value rule of the fit kernels (depth_at)
template <typename DT>
__global__ __launch_bounds__(256) void unpack_depth16_kernel(const DT* __restrict__ src, long long plane_stride, int P, int H, int W_in,
                                                             int W, DepthCvt<DT> cv, float* __restrict__ out) {
  const long long total = (long long)P * H * W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / W;
    const int c = (int)(i - row * W);
    const long long pl = row / H;
    const int r = (int)(row - pl * H);
    out[i] = depth_at<DT>(src + pl * plane_stride, (long long)r * W_in + c, cv);
  }
}

int grid_for(long long items) {
  const long long want = (items + 255) / 256;
  return (int)(want < 1 ? 1 : (want < 16384 ? want : 16384));
}
}  // namespace

extern "C" {

int la3d_pack_depth16(const float* depth, int64_t plane_stride, int P, int H, int W, int W_out, int dtype, float scale, void* out,
                      int64_t out_plane_stride, void* stream) {
  if (dtype != LA3D_DTYPE_F16 && dtype != LA3D_DTYPE_U16) return refuse("la3d_pack_depth16", "unknown dtype (LA3D_DTYPE_F16 or LA3D_DTYPE_U16)");
  if (dtype == LA3D_DTYPE_U16 && !(scale > 0.0f && scale <= 3.4028234663852886e38f))
    return refuse("la3d_pack_depth16", "scale must be finite and > 0");
  if (P < 0 || H <= 0 || W <= 0 || W_out < W || (long long)H * W_out > (1LL << 28) || plane_stride < 0 ||
      (P > 0 && (!depth || !out || (reinterpret_cast<uintptr_t>(depth) & 3) || (reinterpret_cast<uintptr_t>(out) & 1))) ||
      (P > 1 && (plane_stride < (long long)H * W || out_plane_stride < (long long)H * W_out)))
    return refuse("la3d_pack_depth16", "bad argument (W_out >= W, plane strides >= the planes, depth 4-byte and out 2-byte aligned)");
  if (P == 0) return LA3D_SUCCESS;
  const int vec = (W_out % 8 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (P == 1 || out_plane_stride % 8 == 0)) ? 1 : 0;
  const int blocks = grid_for((long long)P * H * ((W_out + 7) / 8));
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned short* o = static_cast<unsigned short*>(out);
  if (dtype == LA3D_DTYPE_F16)
    hipLaunchKernelGGL((pack_depth16_kernel<LA3D_DTYPE_F16>), dim3(blocks), dim3(256), 0, s, depth, (long long)plane_stride, P, H, W, W_out, scale, o,
                       (long long)out_plane_stride, vec);
  else
    hipLaunchKernelGGL((pack_depth16_kernel<LA3D_DTYPE_U16>), dim3(blocks), dim3(256), 0, s, depth, (long long)plane_stride, P, H, W, W_out, scale, o,
                       (long long)out_plane_stride, vec);
  return check_launch("pack_depth16_kernel");
}

int la3d_unpack_depth16(const la3d_depth16* src, int P, int H, int W_in, int W, float* out, void* stream) {
  if (!src || src->struct_size < (int32_t)sizeof(la3d_depth16)) return refuse("la3d_unpack_depth16", "bad struct_size");
  if (src->dtype != LA3D_DTYPE_F16 && src->dtype != LA3D_DTYPE_U16)
    return refuse("la3d_unpack_depth16", "unknown dtype (LA3D_DTYPE_F16 or LA3D_DTYPE_U16)");
  if (src->dtype == LA3D_DTYPE_U16 ? (!(src->scale > 0.0f && src->scale <= 3.4028234663852886e38f) || (src->flags & ~LA3D_DEPTH_ZERO_IS_HOLE))
                                   : src->flags != 0)
    return refuse("la3d_unpack_depth16", "U16 needs a finite scale > 0 and flags LA3D_DEPTH_ZERO_IS_HOLE or 0; F16 needs flags 0");
  if (P < 0 || H <= 0 || W <= 0 || W_in < W || (long long)H * W_in > (1LL << 28) || src->plane_stride < 0 ||
      (P > 0 && (!src->planes || !out || (reinterpret_cast<uintptr_t>(src->planes) & 1))) ||
      (P > 1 && src->plane_stride != 0 && src->plane_stride < (long long)H * W_in))
    return refuse("la3d_unpack_depth16", "bad argument (W <= W_in, plane_stride 0 or >= H*W_in, planes 2-byte aligned)");
  if (P == 0) return LA3D_SUCCESS;
  const int blocks = grid_for((long long)P * H * W);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (src->dtype == LA3D_DTYPE_F16) {
    hipLaunchKernelGGL((unpack_depth16_kernel<d_f16>), dim3(blocks), dim3(256), 0, s, static_cast<const d_f16*>(src->planes),
                       (long long)src->plane_stride, P, H, W_in, W, DepthCvt<d_f16>{}, out);
  } else {
    DepthCvt<d_u16> cv;
    cv.scale = src->scale; cv.hole = (src->flags & LA3D_DEPTH_ZERO_IS_HOLE) ? 1 : 0;
    hipLaunchKernelGGL((unpack_depth16_kernel<d_u16>), dim3(blocks), dim3(256), 0, s, static_cast<const d_u16*>(src->planes),
                       (long long)src->plane_stride, P, H, W_in, W, cv, out);
  }
  return check_launch("unpack_depth16_kernel");
}

}  // extern "C"
