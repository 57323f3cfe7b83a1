// la3d_depth_gate.hip - the depth gate on bit planes (include/la3d.h "depth gate on bit planes"): a mask's pixels whose depth is not
// finite, lies outside [near, far] or lies further from the mask's median depth than max(k * MAD, min_band) are dropped before the fit
// takes every set pixel.  Kernel and C entry in one unit; the two medians are the exact selection of la3d_select.hpp.
#include <cmath>
#include <cstdint>
#include <cstddef>

#include "la3d_bitplanes.hpp"
#include "la3d_select.hpp"

using namespace la3d;

namespace {
struct GateArgs {
  const float* depth; long long depth_stride; const int* image_index;
  const unsigned* bits; long long bits_stride;
  unsigned* out; long long out_stride;
  int* counts; float* levels;
  int W, fw, HW, nwords, vec;
  float k, min_band, near, far;
};

// the VALUES of la3d_select.hpp: the depth itself, then its distance from the median (one float32 subtraction)
struct DepthValue {
  const float* d;
  typedef float In;
  __device__ float idle() const { return 0.f; }
  __device__ float load(int i) const { return d[i]; }
  __device__ float value(float x) const { return x; }
};
struct DeviationValue {
  const float* d; float med;
  typedef float In;
  __device__ float idle() const { return 0.f; }
  __device__ float load(int i) const { return d[i]; }
  __device__ float value(float x) const { return fabsf(x - med); }
};

constexpr int DG_U = 4;   // chunks in flight per wave in the two passes over every chunk of the plane

// One pass over every 64-pixel chunk of the bit image in LDS, a wave per chunk: the lanes whose bit is set load their depth, TEST
// says which of them stay, and the chunk's two words are replaced by the answer.  A wave reads and writes only the words of its own
// chunks, and chunks without a set bit cost two LDS reads.  Returns, in every lane of the wave, the pixels this wave kept; *had (if
// given): the pixels it met.  COLUMNS: the bits of the columns >= fw count as not set (the first pass: the input plane as it came).
template <bool COLUMNS, class TEST>
__device__ inline unsigned gate_pass(const float* __restrict__ dp, unsigned* bits, int nwords, int nchunks, int W, int fw, const TEST& test,
                                     unsigned* had, int wave, int lane) {
  unsigned kept = 0, met = 0;
  for (int c0 = wave * DG_U; c0 < nchunks; c0 += (RM_NT / 64) * DG_U) {
    float d[DG_U];
    unsigned on[DG_U];
#pragma unroll
    for (int u = 0; u < DG_U; ++u) {
      on[u] = 0; d[u] = 0.f;
      const int c = c0 + u;
      if (c < nchunks) {
        on[u] = chunk_bit(bits, nwords, c, lane);
        const int p = c * 64 + lane;              // (< H * W where the bit is set: the tail of the last word is clear in LDS)
        if (COLUMNS && on[u] && p % W >= fw) on[u] = 0;
        if (on[u]) d[u] = dp[p];
      }
    }
#pragma unroll
    for (int u = 0; u < DG_U; ++u) {
      const int c = c0 + u;
      if (c >= nchunks) continue;                 // uniform
      const unsigned long long in = __ballot(on[u] != 0);
      const unsigned long long stay = __ballot(on[u] != 0 && test(d[u]));
      met += (unsigned)__popcll(in); kept += (unsigned)__popcll(stay);
      if (lane == 0) {
        bits[2 * c] = (unsigned)stay;
        if (2 * c + 1 < nwords) bits[2 * c + 1] = (unsigned)(stay >> 32);
      }
    }
  }
  if (had) *had = met;
  return kept;
}

// One 512-thread workgroup per instance:
//   copy    the plane goes into LDS once (16-byte loads where base and stride allow); nothing reads the input plane afterwards, so
//           the output may be the input
//   valid   pass over every chunk: bit set, image column, depth finite and inside [near, far] -> the bit image of the VALID pixels
//   med     np.median of the valid depths, mad = np.median of |depth - med| (re-derived from memory): two exact selections
//   gate    pass over every chunk: |depth - med| <= thr -> the bit image of the KEPT pixels; then all words of the plane are stored
//           from LDS (coalesced) - the bits of the columns >= frame_width and beyond H * W are zero because no pass ever set them
// Integer LDS atomics only (counters, histograms): every output is a count or a selection and depends on neither their order nor the
// rest of the batch.
__global__ __launch_bounds__(RM_NT) void depth_gate_kernel(const GateArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  unsigned* hist = bits + ((a.nwords + 3) & ~3);
  unsigned* h1 = hist + RM_CAP;
  unsigned* bsum = h1 + 1024;
  unsigned* misc = bsum + 256;                   // masked_median's, but [6]: the number of active chunks
  unsigned* cnt = misc + 16;                     // [0] area_in, [1] n_valid, [2] area_out  ([3..7]: unused)
  unsigned short* clist = reinterpret_cast<unsigned short*>(cnt + 8);   // ids of the 64-pixel chunks holding a valid pixel
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, inst = blockIdx.x;
  const float* dp = a.depth + (long long)(a.image_index ? a.image_index[inst] : inst) * a.depth_stride;
  const int nchunks = (a.HW + 63) >> 6;
  if (tid < 8) cnt[tid] = 0u;
  if (tid == 0) misc[6] = 0u;
  bits_plane_to_lds<RM_NT>(a.bits + (long long)inst * a.bits_stride, bits, a.nwords, a.HW, a.vec, tid);
  __syncthreads();
  {
    const float near = a.near, far = a.far;
    unsigned met = 0;
    const auto valid = [&](float d) { return finite_f32(d) && d >= near && d <= far; };
    const unsigned kept = a.fw < a.W ? gate_pass<true>(dp, bits, a.nwords, nchunks, a.W, a.fw, valid, &met, wave, lane)
                                     : gate_pass<false>(dp, bits, a.nwords, nchunks, a.W, a.fw, valid, &met, wave, lane);
    if (lane == 0) { atomicAdd(&cnt[0], met); atomicAdd(&cnt[1], kept); }
  }
  __syncthreads();
  const unsigned n = cnt[1];
  float med = NAN, mad = NAN, thr = NAN;
  if (n != 0) {                          // uniform
    list_active_chunks(bits, a.nwords, nchunks, clist, &misc[6], tid);
    __syncthreads();
    const int nact = (int)misc[6];
    med = masked_median(DepthValue{dp}, n, bits, a.nwords, clist, nact, hist, h1, bsum, misc, tid);
    mad = masked_median(DeviationValue{dp, med}, n, bits, a.nwords, clist, nact, hist, h1, bsum, misc, tid);
    thr = fmaxf(a.k * mad, a.min_band);  // one float32 product
    const float m = med, t = thr;
    const unsigned kept = gate_pass<false>(dp, bits, a.nwords, nchunks, a.W, a.fw, [&](float d) { return fabsf(d - m) <= t; }, nullptr, wave, lane);
    if (lane == 0) atomicAdd(&cnt[2], kept);
    __syncthreads();
  }
  if (a.out) {                           // every word of the plane, from LDS
    unsigned* out = a.out + (long long)inst * a.out_stride;
    for (int w = tid; w < a.nwords; w += RM_NT) out[w] = bits[w];
  }
  if (tid == 0) {
    if (a.counts) { int* c = a.counts + (long long)inst * 3; c[0] = (int)cnt[0]; c[1] = (int)n; c[2] = (int)cnt[2]; }
    if (a.levels) { float* l = a.levels + (long long)inst * 3; l[0] = med; l[1] = mad; l[2] = thr; }
  }
}

// the LDS of one workgroup: the bit image, what masked_median works in, the counters, the chunk list
inline long long gate_lds_bytes(long long HW) {
  const long long nw = (HW + 31) / 32;
  return ((nw + 3) & ~3LL) * 4 + (long long)(RM_WORK_WORDS + 8) * 4 + ((HW + 63) / 64) * 2 + 16;
}
static_assert(((819200 / 32 + 3) & ~3) * 4 + (RM_WORK_WORDS + 8) * 4 + (819200 / 64) * 2 + 16 <= 160 * 1024, "819200 stored pixels fit");
}  // namespace

extern "C" {

int la3d_depth_gate_bits(const la3d_depth_gate_args* args) {
  const char* who = "la3d_depth_gate_bits";
  if (!args || args->struct_size != (int32_t)sizeof(la3d_depth_gate_args)) return refuse(who, "NULL block or a struct_size that is not sizeof(la3d_depth_gate_args)");
  const la3d_depth_gate_args& a = *args;
  if (a.B < 0 || a.H <= 0 || a.W <= 0) return refuse(who, "bad argument (B >= 0, H, W > 0)");
  if (a.frame_width < 0 || a.frame_width > a.W) return refuse(who, "frame_width must lie in [0, W] (0 = W)");
  if (!(a.k >= 0.f) || !std::isfinite(a.k)) return refuse(who, "k must be finite and >= 0");
  if (!(a.min_band >= 0.f) || !std::isfinite(a.min_band)) return refuse(who, "min_band must be finite and >= 0");
  if (a.near != a.near || a.far != a.far) return refuse(who, "near and far must not be NaN");
  if (a.reserved != 0) return refuse(who, "reserved must be 0");
  const long long HW = (long long)a.H * a.W, words = (HW + 31) / 32;
  if (a.depth_plane_stride < 0 || (a.depth_plane_stride != 0 && a.depth_plane_stride < HW))
    return refuse(who, "depth_plane_stride must be 0 (one shared plane) or at least H * W");
  if (a.bits_plane_stride < 0 || (a.bits_plane_stride != 0 && a.bits_plane_stride < words)) 
    return refuse(who, "bits_plane_stride is smaller than la3d_mask_bits_words(H, W)");
  if (a.out_plane_stride < 0 || (a.out_plane_stride != 0 && a.out_plane_stride < words))
    return refuse(who, "out_plane_stride is smaller than la3d_mask_bits_words(H, W)");
  if (gate_lds_bytes(HW) > 160 * 1024)
    return refuse(who, "frame too large for the LDS bit image (H * W up to 857728 stored pixels)", LA3D_ERR_UNSUPPORTED);
  if (a.B == 0) return LA3D_SUCCESS;
  if (!a.out_bits && !a.counts && !a.levels) return refuse(who, "nothing to do: out_bits, counts and levels are all NULL");
  if (!a.depth || !a.mask_bits) return refuse(who, "depth and mask_bits must not be NULL");
  if ((at(a.depth) | at(a.image_index) | at(a.mask_bits) | at(a.out_bits) | at(a.counts) | at(a.levels)) & 3)
    return refuse(who, "depth, image_index, mask_bits, out_bits, counts or levels not a 4-byte aligned pointer");
  const long long bs = a.bits_plane_stride ? a.bits_plane_stride : words, os = a.out_plane_stride ? a.out_plane_stride : words;
  // in place: every word of the input is in LDS before a word is stored, so the output may be EXACTLY the input; planes that share
  // bytes any other way belong to different workgroups
  if (a.out_bits && !(a.out_bits == a.mask_bits && os == bs) &&
      planes_overlap(a.mask_bits, (uintptr_t)a.B * (uintptr_t)bs, a.out_bits, (uintptr_t)a.B * (uintptr_t)os))
    return refuse(who, "the input planes and the output planes overlap without being the same planes (in place: out_bits == mask_bits, equal strides)");
  GateArgs g = {};
  g.depth = a.depth; g.depth_stride = a.depth_plane_stride; g.image_index = a.image_index;
  g.bits = a.mask_bits; g.bits_stride = bs; g.out = a.out_bits; g.out_stride = os;
  g.counts = a.counts; g.levels = a.levels;
  g.W = a.W; g.fw = a.frame_width ? a.frame_width : a.W; g.HW = (int)HW; g.nwords = (int)words;
  g.vec = ((at(a.mask_bits) & 15) == 0 && bs % 4 == 0) ? 1 : 0;
  g.k = a.k; g.min_band = a.min_band; g.near = a.near; g.far = a.far;
  allow_big_lds(reinterpret_cast<const void*>(depth_gate_kernel));
  hipLaunchKernelGGL(depth_gate_kernel, dim3((unsigned)a.B), dim3(RM_NT), (size_t)gate_lds_bytes(HW), static_cast<hipStream_t>(a.stream), g);
  return check_launch("depth_gate_kernel");
}

}  // extern "C"
