// la3d_depth_gate.hip - the depth gate on bit planes (include/la3d.h "depth gate on bit planes"): a mask's pixels whose depth is not
// finite, lies outside [near, far] or lies further from the mask's median depth than max(k * MAD, min_band) are dropped before the fit
// takes every set pixel.  Kernel and C entries in one unit; the two medians are the exact selection of la3d_select.hpp.  ONE kernel
// text serves the uniform form (la3d_depth_gate_bits: planes of one frame size, float32 depth) and the frames form
// (la3d_depth_gate_bits_frames: every row the plane of its own image's frame, depth float32, float16 or uint16 where it lies).
#include <cmath>
#include <cstdint>
#include <cstddef>

#include "la3d_bitplanes.hpp"
#include "la3d_select.hpp"

using namespace la3d;

namespace {
struct GateArgs {
  const void* depth; long long depth_stride; const int* image_index;   // depth: elements of the kernel's DT
  const unsigned* bits; long long bits_stride;
  unsigned* out; long long out_stride;
  int* counts; float* levels;
  int W, fw, HW, nwords, vec;      // frames form: HW and nwords are those of the BOUNDS (they place the LDS regions), W the bounds' pitch
  float k, min_band, near, far;
};
// what the frames form adds: the plane locator, the bound on the rows and the elements of the depth buffer
struct GateFrames { FramesPlanes planes; int max_h; long long depth_elems; };

// the VALUES of la3d_select.hpp: the depth itself, then its distance from the median (one float32 subtraction).  16-bit planes
// (d_f16, d_u16) load the stored word and make the float32 by the rule of the fit (depth_bits: F16 exact; U16 ONE rounded product,
// a stored 0 a NaN with `hole`).  `__fmul_rn` is a plain product for hipcc: what keeps the U16 product out of an fma with the
// subtraction behind it is the pragma on that subtraction - without it |x * scale - med| is rounded once, not twice.
template <typename DT> struct DepthValue {
  const DT* d; DepthCvt<DT> cv;
  typedef unsigned short In;
  __device__ In idle() const { return 0; }
  __device__ In load(int i) const { return d[i].b; }
  __device__ float value(In x) const { return __uint_as_float(depth_bits<DT>((unsigned)x, cv)); }
};
template <typename DT> struct DeviationValue {
  const DT* d; DepthCvt<DT> cv; float med;
  typedef unsigned short In;
  __device__ In idle() const { return 0; }
  __device__ In load(int i) const { return d[i].b; }
  __device__ float value(In x) const {
#pragma clang fp contract(off)
    return fabsf(__uint_as_float(depth_bits<DT>((unsigned)x, cv)) - med);
  }
};
template <> struct DepthValue<float> {
  const float* d; DepthCvt<float> cv;
  typedef float In;
  __device__ float idle() const { return 0.f; }
  __device__ float load(int i) const { return d[i]; }
  __device__ float value(float x) const { return x; }
};
template <> struct DeviationValue<float> {
  const float* d; DepthCvt<float> cv; float med;
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
// The depth comes through a DepthValue: its loads are issued for DG_U chunks before any is converted and tested.
template <bool COLUMNS, class V, class TEST>
__device__ inline unsigned gate_pass(const V& dv, unsigned* bits, int nwords, int nchunks, int W, int fw, const TEST& test,
                                     unsigned* had, int wave, int lane) {
  unsigned kept = 0, met = 0;
  for (int c0 = wave * DG_U; c0 < nchunks; c0 += (RM_NT / 64) * DG_U) {
    typename V::In d[DG_U];
    unsigned on[DG_U];
#pragma unroll
    for (int u = 0; u < DG_U; ++u) {
      on[u] = 0; d[u] = dv.idle();
      const int c = c0 + u;
      if (c < nchunks) {
        on[u] = chunk_bit(bits, nwords, c, lane);
        const int p = c * 64 + lane;              // (< H * W where the bit is set: the tail of the last word is clear in LDS)
        if (COLUMNS && on[u] && p % W >= fw) on[u] = 0;
        if (on[u]) d[u] = dv.load(p);
      }
    }
#pragma unroll
    for (int u = 0; u < DG_U; ++u) {
      const int c = c0 + u;
      if (c >= nchunks) continue;                 // uniform
      const unsigned long long in = __ballot(on[u] != 0);
      const unsigned long long stay = __ballot(on[u] != 0 && test(dv.value(d[u])));
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
// FRAMES: row `inst` is the plane of its OWN image's frame.  Every value that decides whether and where something is read or written
// is wave-uniform and checked before an address is formed from it, in this order: frames_source (image index, frame row, plane
// offset, the plane's end inside bits_words), frames_dest (with planes to store: the output offset and its end inside out_words),
// then the depth plane's end inside the depth buffer.  A refused row reads no plane or depth word, writes no plane word and gets
// counts -2, 0, 0 and NaN levels, addressed by `inst` alone.  H, pitch, frame_width, words and chunks are then the row's; the LDS
// regions stay where the BOUNDS put them (a.nwords, a.HW), which is what the launch reserved.
// DT: the element of the depth planes - float (the uniform entry: the code it always was), d_f16, d_u16 with their DepthCvt.
// (flatten: two instantiations share the float selection, and a function with two callers is no longer inlined by itself - the
// uniform kernel then calls it, with twice the registers and a stack; flattened, it is the instruction stream it was.)
template <bool FRAMES, typename DT>
__global__ __launch_bounds__(RM_NT) __attribute__((flatten)) void depth_gate_kernel(const GateArgs a, const GateFrames fr, const DepthCvt<DT> cv) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  unsigned* hist = bits + ((a.nwords + 3) & ~3);
  unsigned* h1 = hist + RM_CAP;
  unsigned* bsum = h1 + 1024;
  unsigned* misc = bsum + 256;                   // masked_median's, but [6]: the number of active chunks
  unsigned* cnt = misc + 16;                     // [0] area_in, [1] n_valid, [2] area_out  ([3..7]: unused)
  unsigned short* clist = reinterpret_cast<unsigned short*>(cnt + 8);   // ids of the 64-pixel chunks holding a valid pixel
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, inst = blockIdx.x;
  const DT* dp;
  const unsigned* src;
  long long ooff = 0;                            // frames form: words from a.out to the row's plane (with planes to store)
  int W, fw, HW, nwords, vec;
  if constexpr (FRAMES) {
    FramesWork f;
    bool ok = frames_source(fr.planes, a.bits, fr.max_h, a.W, inst, &f);
    if (ok && a.out) ok = frames_dest(fr.planes, inst, f.nwords, &ooff);
    if (ok) ok = f.r.off <= fr.depth_elems - (long long)f.r.H * f.r.W;
    if (!ok) {                           // uniform
      if (tid == 0) {
        if (a.counts) { int* c = a.counts + (long long)inst * 3; c[0] = -2; c[1] = 0; c[2] = 0; }
        if (a.levels) { float* l = a.levels + (long long)inst * 3; l[0] = NAN; l[1] = NAN; l[2] = NAN; }
      }
      return;
    }
    W = f.r.W; fw = f.r.fw; HW = f.r.H * f.r.W; nwords = f.nwords; vec = 1;   // (bits 16-byte aligned, the offset a multiple of 4)
    dp = static_cast<const DT*>(a.depth) + f.r.off;
    src = a.bits + f.off;
  } else {
    W = a.W; fw = a.fw; HW = a.HW; nwords = a.nwords; vec = a.vec;
    dp = static_cast<const DT*>(a.depth) + (long long)(a.image_index ? a.image_index[inst] : inst) * a.depth_stride;
    src = a.bits + (long long)inst * a.bits_stride;
  }
  const int nchunks = (HW + 63) >> 6;
  if (tid < 8) cnt[tid] = 0u;
  if (tid == 0) misc[6] = 0u;
  bits_plane_to_lds<RM_NT>(src, bits, nwords, HW, vec, tid);
  __syncthreads();
  const DepthValue<DT> dv{dp, cv};
  {
    const float near = a.near, far = a.far;
    unsigned met = 0;
    const auto valid = [&](float d) { return finite_f32(d) && d >= near && d <= far; };
    const unsigned kept = fw < W ? gate_pass<true>(dv, bits, nwords, nchunks, W, fw, valid, &met, wave, lane)
                                 : gate_pass<false>(dv, bits, nwords, nchunks, W, fw, valid, &met, wave, lane);
    if (lane == 0) { atomicAdd(&cnt[0], met); atomicAdd(&cnt[1], kept); }
  }
  __syncthreads();
  const unsigned n = cnt[1];
  float med = NAN, mad = NAN, thr = NAN;
  if (n != 0) {                          // uniform
    list_active_chunks(bits, nwords, nchunks, clist, &misc[6], tid);
    __syncthreads();
    const int nact = (int)misc[6];
    med = masked_median(dv, n, bits, nwords, clist, nact, hist, h1, bsum, misc, tid);
    mad = masked_median(DeviationValue<DT>{dp, cv, med}, n, bits, nwords, clist, nact, hist, h1, bsum, misc, tid);
    thr = fmaxf(a.k * mad, a.min_band);  // one float32 product
    const float m = med, t = thr;
    const auto inside = [&](float d) {   // (one float32 subtraction of the ROUNDED depth: see DeviationValue)
#pragma clang fp contract(off)
      return fabsf(d - m) <= t;
    };
    const unsigned kept = gate_pass<false>(dv, bits, nwords, nchunks, W, fw, inside, nullptr, wave, lane);
    if (lane == 0) atomicAdd(&cnt[2], kept);
    __syncthreads();
  }
  if (a.out) {                           // every word of the plane, from LDS
    unsigned* out = a.out + (FRAMES ? ooff : (long long)inst * a.out_stride);
    for (int w = tid; w < nwords; w += RM_NT) out[w] = bits[w];
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

// one launch of either form: B workgroups, the dynamic LDS of HW stored pixels (frames form: the bounds')
template <bool FRAMES, typename DT>
void launch_gate(const GateArgs& g, const GateFrames& fr, const DepthCvt<DT>& cv, int B, long long HW, void* stream) {
  allow_big_lds(reinterpret_cast<const void*>(depth_gate_kernel<FRAMES, DT>));
  hipLaunchKernelGGL((depth_gate_kernel<FRAMES, DT>), dim3((unsigned)B), dim3(RM_NT), (size_t)gate_lds_bytes(HW), static_cast<hipStream_t>(stream), g, fr, cv);
}
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
  launch_gate<false, float>(g, GateFrames{}, DepthCvt<float>{}, a.B, HW, a.stream);
  return check_launch("depth_gate_kernel");
}

int la3d_depth_gate_bits_frames(const la3d_depth_gate_frames_args* args) {
  const char* who = "la3d_depth_gate_bits_frames";
  static_assert(sizeof(la3d_depth_gate_frames_args) == 152, "la3d_depth_gate_frames_args is part of the ABI");
  if (!args || args->struct_size != (int32_t)sizeof(la3d_depth_gate_frames_args))
    return refuse(who, "NULL block or a struct_size that is not sizeof(la3d_depth_gate_frames_args)");
  const la3d_depth_gate_frames_args& a = *args;
  if (a.B < 0 || a.P < 0 || a.H <= 0 || a.W <= 0) return refuse(who, SIZES_FRAMES);
  if (!(a.k >= 0.f) || !std::isfinite(a.k)) return refuse(who, "k must be finite and >= 0");
  if (!(a.min_band >= 0.f) || !std::isfinite(a.min_band)) return refuse(who, "min_band must be finite and >= 0");
  if (a.near != a.near || a.far != a.far) return refuse(who, "near and far must not be NaN");
  if (a.reserved != 0) return refuse(who, "reserved must be 0");
  if ((a.depth ? 1 : 0) + (a.depth16 ? 1 : 0) != 1) return refuse(who, "give exactly one of depth / depth16");
  const void* planes = a.depth;
  int dtype = LA3D_DTYPE_F32;
  DepthCvt<d_u16> cv16;
  if (a.depth16) {                       // the rules of la3d_fit_instances_frames_depth16
    const la3d_depth16* d = a.depth16;
    if (d->struct_size < (int32_t)sizeof(la3d_depth16)) return refuse(who, "bad struct_size of la3d_depth16");
    if (d->dtype != LA3D_DTYPE_F16 && d->dtype != LA3D_DTYPE_U16) return refuse(who, "la3d_depth16: unknown dtype (LA3D_DTYPE_F16 or LA3D_DTYPE_U16)");
    if (d->dtype == LA3D_DTYPE_U16 ? (!(d->scale > 0.0f && d->scale <= 3.4028234663852886e38f) || (d->flags & ~LA3D_DEPTH_ZERO_IS_HOLE)) : d->flags != 0)
      return refuse(who, "la3d_depth16: U16 needs a finite scale > 0 and flags LA3D_DEPTH_ZERO_IS_HOLE or 0; F16 needs flags 0");
    if (d->plane_stride != 0) return refuse(who, "la3d_depth16: plane_stride must be 0 (the frame table says where every plane lies)");
    if (!d->planes) return refuse(who, "la3d_depth16: planes is NULL");
    planes = d->planes; dtype = d->dtype;
    if (dtype == LA3D_DTYPE_U16) { cv16.scale = d->scale; cv16.hole = (d->flags & LA3D_DEPTH_ZERO_IS_HOLE) ? 1 : 0; }
  }
  if (a.depth_elems < 0 || a.bits_words < 0 || (a.out_bits && a.out_words < 0))
    return refuse(who, "depth_elems, bits_words and out_words must not be negative");
  if ((at(a.bits) | at(a.out_bits)) & 15) return refuse(who, "bits or out_bits not a 16-byte aligned pointer");
  if (at(planes) & (a.depth16 ? 7 : 15)) return refuse(who, "the depth buffer must be 16-byte (16-bit planes: 8-byte) aligned");
  if ((at(a.bits_offsets) | at(a.out_offsets) | at(a.frames)) & 7) return refuse(who, "bits_offsets, out_offsets or frames not an 8-byte aligned pointer");
  if ((at(a.image_index) | at(a.counts) | at(a.levels)) & 3) return refuse(who, "image_index, counts or levels not a 4-byte aligned pointer");
  if (!a.out_bits && !a.counts && !a.levels) return refuse(who, "nothing to do: out_bits, counts and levels are all NULL");
  // in place: every word of a row's plane is in LDS before a word of it is stored, so the output may be EXACTLY the input - the same
  // buffer, its length and the very offsets; rows whose planes share words any other way belong to different workgroups
  if (a.bits && a.out_bits && !(a.out_bits == a.bits && a.out_words == a.bits_words && a.out_offsets == a.bits_offsets) &&
      planes_overlap(a.bits, (uintptr_t)a.bits_words, a.out_bits, (uintptr_t)a.out_words))
    return refuse(who, "the input buffer and the output buffer overlap without being the same planes (in place: out_bits == bits, out_words == bits_words, out_offsets == bits_offsets)");
  if (a.B > 0) {
    if (!a.bits || !a.bits_offsets || !a.image_index || (!a.frames && a.P > 0)) return refuse(who, "NULL bits, bits_offsets, image_index or frames");
    if (a.out_bits && !a.out_offsets) return refuse(who, "out_offsets must not be NULL with out_bits");
  }
  const long long HW = bounds_words(a.H, a.W) * 32;
  if (gate_lds_bytes(HW) > 160 * 1024)
    return refuse(who, "bounds too large for the LDS bit image (H * roundup32(W) up to 857728 stored pixels)", LA3D_ERR_UNSUPPORTED);
  if (a.B == 0) return LA3D_SUCCESS;
  GateArgs g = {};
  g.depth = planes; g.image_index = a.image_index;
  g.bits = a.bits; g.out = a.out_bits;
  g.counts = a.counts; g.levels = a.levels;
  g.W = (int)(HW / a.H); g.fw = g.W; g.HW = (int)HW; g.nwords = (int)(HW / 32); g.vec = 1;   // the bounds: a row's own geometry is formed per workgroup
  g.k = a.k; g.min_band = a.min_band; g.near = a.near; g.far = a.far;
  GateFrames fr = {};
  fr.planes.offsets = reinterpret_cast<const long long*>(a.bits_offsets); fr.planes.out_offsets = reinterpret_cast<const long long*>(a.out_offsets);
  fr.planes.frames = a.frames; fr.planes.image_index = a.image_index; fr.planes.P = a.P;   // (P == 0: every row is refused before a frame row is addressed)
  fr.planes.bits_words = a.bits_words; fr.planes.out_words = a.out_bits ? a.out_words : 0;
  fr.max_h = a.H; fr.depth_elems = a.depth_elems;
  if (dtype == LA3D_DTYPE_F16) launch_gate<true, d_f16>(g, fr, DepthCvt<d_f16>{}, a.B, HW, a.stream);
  else if (dtype == LA3D_DTYPE_U16) launch_gate<true, d_u16>(g, fr, cv16, a.B, HW, a.stream);
  else launch_gate<true, float>(g, fr, DepthCvt<float>{}, a.B, HW, a.stream);
  return check_launch("depth_gate_kernel");
}

}  // extern "C"
