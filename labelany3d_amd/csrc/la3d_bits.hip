// la3d_bits.hip - masks as bit planes (include/la3d.h "masks as bit planes"): the packers of u8 masks, logits, label maps, COCO run
// lengths, polygons and crop-space masks - each in its uniform and its frames form -, the unpacker and the filter statistics of a bit
// plane.  This unit also owns the family "annotation into an LDS bit image": bits_to_plane and with it la3d_rle_decode /
// la3d_poly_decode, whose kernels the annotation packers repeat with the LDS image kept as the output.
// Shared with the other bit-plane units and stated once, in la3d_bitplanes.hpp: where the planes go (BitsOut), the host check
// (pack_check), the frames prologue of a workgroup (frames_prologue).  The way back out of a plane, the run-length encoder, is
// la3d_rle_encode.hip; morphology is la3d_open.hip.  la3d_masks.hip keeps depth_to_points, row padding and the statistics of u8 planes,
// run lengths and polygons.
#include <cstdint>
#include <cstddef>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "la3d_device.hpp"
#include "la3d_poly.hpp"
#include "la3d_bitplanes.hpp"

using namespace la3d;

namespace {
// bit image in LDS -> u8 plane (0/1), coalesced 16-byte non-temporal stores where the plane allows; NTH threads.  Four bits
// become four bytes with one multiply: bit i of the nibble lands at 8 i through the partial product shifted by 7 i (the 16 partial
// products hit 16 different bit positions: no carries).
template <int NTH>
__device__ inline void bits_to_plane(const unsigned* bits, int HW, unsigned char* o, int tid) {
  const unsigned short* b16 = reinterpret_cast<const unsigned short*>(bits);
  if (HW % 16 == 0 && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
#pragma unroll 4
    for (int g = tid; g < HW / 16; g += NTH) {
      const unsigned pat = b16[g];
      u32x4 v;
      v.x = ((pat & 0xFu) * 0x00204081u) & 0x01010101u;
      v.y = (((pat >> 4) & 0xFu) * 0x00204081u) & 0x01010101u;
      v.z = (((pat >> 8) & 0xFu) * 0x00204081u) & 0x01010101u;
      v.w = (((pat >> 12) & 0xFu) * 0x00204081u) & 0x01010101u;
      __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(o + g * 16));
    }
  } else {
    for (int i = tid; i < HW; i += NTH) o[i] = (bits[i >> 5] >> (i & 31)) & 1u;
  }
}

// mask_utils.decode for a batch (reference src/util.py:367,401-402): run lengths -> u8 planes.  The runs are
// decoded into an LDS bit image (rle_to_bits) and expanded with coalesced 16-byte stores.
__global__ __launch_bounds__(NT_DEC) void rle_decode_kernel(const int* __restrict__ counts, const long long* __restrict__ offsets,
                                                            int H, int W, int nwords, int scan_words, unsigned char* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  unsigned* wtot = bits + nwords;
  const int tid = threadIdx.x;
  const long long o0 = offsets[blockIdx.x];
  (void)rle_to_bits<NT_DEC>(counts + o0, (int)(offsets[blockIdx.x + 1] - o0), bits, nwords, H, W, wtot, tid, wtot + 16, scan_words);
  bits_to_plane<NT_DEC>(bits, H * W, out + (long long)blockIdx.x * H * W, tid);
}

// create_boolean_mask_from_polygon for a batch (reference src/util.py:386-400): polygon parts -> u8 planes.  Dynamic LDS:
// bit image (16-aligned), side stage, flags.
__global__ __launch_bounds__(NT_DEC) void poly_decode_kernel(const int* __restrict__ xy, const long long* __restrict__ ring_off,
                                                          const long long* __restrict__ inst_rings, int H, int W, int nwords,
                                                          unsigned char* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  const size_t bit_bytes = ((size_t)nwords * 4 + 15) & ~(size_t)15;
  PolySide* stage = reinterpret_cast<PolySide*>(smem + bit_bytes);
  unsigned* flags = reinterpret_cast<unsigned*>(smem + bit_bytes + POLY_STAGE_BYTES);
  const int tid = threadIdx.x;
  (void)poly_to_bits<NT_DEC>(xy, ring_off, inst_rings[blockIdx.x], inst_rings[blockIdx.x + 1], stage, flags, bits, nwords, H, W, tid);
  bits_to_plane<NT_DEC>(bits, H * W, out + (long long)blockIdx.x * H * W, tid);
}

// ---- annotations -> bit planes (la3d_pack_rle_bits / la3d_pack_poly_bits and their frames forms) -----------------------------
// The two decode kernels above with the LDS bit image KEPT as the output: one workgroup of NT_DEC threads per instance decodes into
// LDS (rle_to_bits / poly_to_bits with frame_w / clipW: the bits of the padding columns are zero) and streams the words to the
// instance's plane - an eighth of the bytes of the u8 plane.  The workgroup owns its instance: the area is reduced inside it and
// stored by one lane (no atomic, no clear kernel).
// bit image in LDS -> the plane's nwords words, exactly those: 16-byte non-temporal stores (vec: the plane's base is 16-byte
// aligned) and up to three words of tail, or word by word.  Then area[b] = the popcount of the words as written.  red: LDS, NTH / 64 ints.
template <int NTH>
__device__ inline void lds_to_bits_plane(const unsigned* bits, const PlaneGeo& g, int* red, int* __restrict__ area, int b, int tid) {
  int n = 0;
  if (g.vec) {   // uniform
    const int ng = g.nwords >> 2;
    const u32x4* s4 = reinterpret_cast<const u32x4*>(bits);
    u32x4* o4 = reinterpret_cast<u32x4*>(g.out);
#pragma unroll 4
    for (int q = tid; q < ng; q += NTH) {
      const u32x4 w = s4[q];
      __builtin_nontemporal_store(w, o4 + q);
      n += (__popc(w.x) + __popc(w.y)) + (__popc(w.z) + __popc(w.w));
    }
    const int r = ng * 4 + tid;   // the up to three words behind the last whole group
    if (tid < 4 && r < g.nwords) {
      const unsigned w = bits[r];
      g.out[r] = w;
      n += __popc(w);
    }
  } else {
    for (int i = tid; i < g.nwords; i += NTH) {
      const unsigned w = bits[i];
      g.out[i] = w;
      n += __popc(w);
    }
  }
  if (!area) return;   // uniform
  n = wave_sum_i(n);
  if ((tid & 63) == 0) red[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < NTH / 64; ++w) s += red[w];
    area[b] = s;
  }
}

// Dynamic LDS: the bit image (lds_words), 16 words of wave totals, the block totals of the column scan (scan_words) - the layout
// of rle_decode_kernel, sized by the call's bounds.
template <bool FRAMES>
__global__ __launch_bounds__(NT_DEC) void pack_rle_bits_kernel(const int* __restrict__ counts, const long long* __restrict__ offsets,
                                                               int scan_words, const BitsOut c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int red[NT_DEC / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  PlaneGeo g;
  if (!plane_geometry<FRAMES>(c, b, &g)) {   // (uniform) refused: no plane word, area 0
    if (tid == 0 && c.area) c.area[b] = 0;
    return;
  }
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  unsigned* wtot = bits + c.lds_words;
  const long long o0 = offsets[b];
  (void)rle_to_bits<NT_DEC>(counts + o0, (int)(offsets[b + 1] - o0), bits, g.nwords, g.H, g.W, wtot, tid, wtot + 16, scan_words, g.fw);
  __syncthreads();
  lds_to_bits_plane<NT_DEC>(bits, g, red, c.area, b, tid);
}

// Dynamic LDS: bit image (16-aligned), side stage, flags - the layout of poly_decode_kernel, sized by the call's bounds.
template <bool FRAMES>
__global__ __launch_bounds__(NT_DEC) void pack_poly_bits_kernel(const int* __restrict__ xy, const long long* __restrict__ ring_off,
                                                                const long long* __restrict__ inst_rings, const BitsOut c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int red[NT_DEC / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  PlaneGeo g;
  if (!plane_geometry<FRAMES>(c, b, &g)) {   // (uniform) refused: no plane word, area 0
    if (tid == 0 && c.area) c.area[b] = 0;
    return;
  }
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  const size_t bit_bytes = ((size_t)c.lds_words * 4 + 15) & ~(size_t)15;
  PolySide* stage = reinterpret_cast<PolySide*>(smem + bit_bytes);
  unsigned* flags = reinterpret_cast<unsigned*>(smem + bit_bytes + POLY_STAGE_BYTES);
  (void)poly_to_bits<NT_DEC>(xy, ring_off, inst_rings[b], inst_rings[b + 1], stage, flags, bits, g.nwords, g.H, g.W, tid, g.fw);
  __syncthreads();
  lds_to_bits_plane<NT_DEC>(bits, g, red, c.area, b, tid);
}

// ------------------------------------------------------------------------------------------
// masks as bit planes (include/la3d.h "masks as bit planes"): packers, unpacker, filter statistics
// ------------------------------------------------------------------------------------------
// element kinds of the packers: a u8 mask (bit = byte != 0) or logits (bit = x > threshold in float32; NaN compares false)
enum { PK_U8 = 0, PK_F32 = 1, PK_F16 = 2, PK_BF16 = 3 };
template <int KIND> struct PackElem;
template <> struct PackElem<PK_U8>   { typedef unsigned char T; };
template <> struct PackElem<PK_F32>  { typedef float T; };
template <> struct PackElem<PK_F16>  { typedef unsigned short T; };
template <> struct PackElem<PK_BF16> { typedef unsigned short T; };

__device__ inline float pk_f16(unsigned h) { return (float)__builtin_bit_cast(_Float16, (unsigned short)h); }
__device__ inline float pk_bf16(unsigned h) { return __uint_as_float(h << 16); }
template <int KIND>
__device__ inline bool pack_pred(typename PackElem<KIND>::T x, float thr) {
  if constexpr (KIND == PK_U8) return x != 0;
  else if constexpr (KIND == PK_F32) return x > thr;
  else if constexpr (KIND == PK_F16) return pk_f16(x) > thr;
  else return pk_bf16(x) > thr;
}
// the bits of the 16 bytes one lane loads: 16 (u8), 8 (f16 / bf16) or 4 (f32) elements, element 0 -> bit 0
template <int KIND>
__device__ inline unsigned pack_group(const u32x4 w, float thr) {
  if constexpr (KIND == PK_U8) {
    return nz16(w.x, w.y, w.z, w.w);
  } else if constexpr (KIND == PK_F32) {
    return (__uint_as_float(w.x) > thr ? 1u : 0u) | (__uint_as_float(w.y) > thr ? 2u : 0u) | (__uint_as_float(w.z) > thr ? 4u : 0u) |
           (__uint_as_float(w.w) > thr ? 8u : 0u);
  } else {
    const unsigned q[4] = {w.x, w.y, w.z, w.w};
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float lo = KIND == PK_F16 ? pk_f16(q[k] & 0xffffu) : pk_bf16(q[k] & 0xffffu);
      const float hi = KIND == PK_F16 ? pk_f16(q[k] >> 16) : pk_bf16(q[k] >> 16);
      r |= (lo > thr ? 1u : 0u) << (2 * k) | (hi > thr ? 1u : 0u) << (2 * k + 1);
    }
    return r;
  }
}

// Vector form (chosen on the host: W_out == W, H*W % 32 == 0, every plane base 16-byte aligned): the plane is one linear run of
// elements, every lane loads 16 bytes (fully coalesced) and the 2 / 4 / 8 neighbouring lanes that share an output word OR their
// pieces together with DPP moves; one lane of each group stores the whole word.  blockIdx.x = plane * chunks + chunk.
template <int KIND>
__global__ __launch_bounds__(256) void pack_bits_vec_kernel(const void* __restrict__ src, long long plane_stride_bytes, float thr, int HW,
                                                            int chunks, unsigned* __restrict__ out, long long out_stride) {
  constexpr int EPL = 16 / (int)sizeof(typename PackElem<KIND>::T);   // elements per lane
  constexpr int LPW = 32 / EPL;                                      // lanes per output word: 2, 4, 8
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const u32x4* s4 = reinterpret_cast<const u32x4*>(static_cast<const unsigned char*>(src) + (long long)b * plane_stride_bytes);
  unsigned* o = out + (long long)b * out_stride;
  const int ngroups = HW / EPL;   // a multiple of LPW
  for (int g0 = chunk * 256; g0 < ngroups; g0 += chunks * 256) {   // uniform trip count: every lane takes part in the DPP steps
    const int g = g0 + (int)threadIdx.x;
    unsigned pat = 0;
    if (g < ngroups) pat = pack_group<KIND>(__builtin_nontemporal_load(s4 + g), thr) << (EPL * (g & (LPW - 1)));
    pat |= (unsigned)dpp_i32<DPP_XOR1>((int)pat);
    if constexpr (LPW >= 4) pat |= (unsigned)dpp_i32<DPP_XOR2>((int)pat);
    if constexpr (LPW >= 8) pat |= (unsigned)dpp_i32<DPP_HALF_MIRROR>((int)pat);
    if (g < ngroups && (g & (LPW - 1)) == 0) o[g / LPW] = pat;
  }
}

// General form: one thread per output word, any stride / alignment / row padding; element (v, u) is read when v < H and u < W.
template <int KIND>
__global__ __launch_bounds__(256) void pack_bits_kernel(const void* __restrict__ src, long long plane_stride_elems, float thr, int H, int W,
                                                        int W_out, int nwords, int chunks, unsigned* __restrict__ out,
                                                        long long out_stride) {
  typedef typename PackElem<KIND>::T T;
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const T* sp = static_cast<const T*>(src) + (long long)b * plane_stride_elems;
  unsigned* o = out + (long long)b * out_stride;
  const long long total = (long long)H * W_out;
  for (int w = chunk * 256 + (int)threadIdx.x; w < nwords; w += chunks * 256) {
    const long long i0 = (long long)w * 32;
    int v = (int)(i0 / W_out), u = (int)(i0 - (long long)v * W_out);
    unsigned pat = 0;
    for (int k = 0; k < 32 && i0 + k < total; ++k) {
      if (u < W && pack_pred<KIND>(sp[(long long)v * W + u], thr)) pat |= 1u << k;
      if (++u == W_out) { u = 0; ++v; }
    }
    o[w] = pat;
  }
}

// bit planes stored W_in pixels wide -> u8 planes [B][H][W] (0 / 1): one thread per four output bytes where W % 4 == 0 (one 32-bit
// store), per byte otherwise
__global__ __launch_bounds__(256) void unpack_mask_bits_kernel(const unsigned* __restrict__ bits, long long stride, int H, int W_in, int W,
                                                               int quads, int chunks, unsigned char* __restrict__ mask) {
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const unsigned* bp = bits + (long long)b * stride;
  unsigned char* mp = mask + (long long)b * H * W;
  const long long HW = (long long)H * W;
  if (quads) {   // uniform
    const int wq = W >> 2;
    const long long nq = HW >> 2;
    for (long long q = (long long)chunk * 256 + threadIdx.x; q < nq; q += (long long)chunks * 256) {
      const int v = (int)(q / wq), u = (int)(q - (long long)v * wq) * 4;
      const long long i = (long long)v * W_in + u;
      const unsigned sh = (unsigned)(i & 31);
      unsigned n = bp[i >> 5] >> sh;
      if (sh > 28) n |= bp[(i >> 5) + 1] << (32 - sh);
      n &= 15u;
      reinterpret_cast<unsigned*>(mp)[q] = (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21);
    }
  } else {
    for (long long q = (long long)chunk * 256 + threadIdx.x; q < HW; q += (long long)chunks * 256) {
      const int v = (int)(q / W), u = (int)(q - (long long)v * W);
      const long long i = (long long)v * W_in + u;
      mp[q] = (unsigned char)((bp[i >> 5] >> (i & 31)) & 1u);
    }
  }
}

// the four filter quantities of one bit plane per workgroup: the plane into LDS (as the fit kernel's phase 0 takes it), then the
// statistics the fused filter computes (bits_filter_stats).  Dynamic LDS: the bit image.
__global__ __launch_bounds__(256) void mask_stats_bits_kernel(const unsigned* __restrict__ planes, long long stride, int vec, int H, int W,
                                                              int frame_w, int nwords, int boundary, int* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  __shared__ int red[5 * 4];
  const int tid = threadIdx.x;
  bits_plane_to_lds<256>(planes + (long long)blockIdx.x * stride, bits, nwords, H * W, vec, tid);
  __syncthreads();
  int st4[4];
  bits_filter_stats<256>(bits, H, frame_w, boundary, red, tid, st4, W);
  if (tid < 4) (stats + (long long)blockIdx.x * 4)[tid] = st4[tid];
}

// ---- masks as label maps ------------------------------------------------------------------
// include/la3d.h "masks as label maps": one (H, W) plane of segment ids per image -> one bit plane per (image, id) row, in the
// format of the packers above.  Both forms hold the 32 labels of an output word in registers and loop over the image's instances,
// so the labels of an image are read once however many instances it has.
enum { LB_U8 = LA3D_LABEL_U8, LB_U16 = LA3D_LABEL_U16, LB_I32 = LA3D_LABEL_I32, LB_RGB8 = LA3D_LABEL_RGB8 };
template <int KIND> struct LabelElem;
template <> struct LabelElem<LB_U8>   { typedef unsigned char T;  static constexpr int BYTES = 1; };
template <> struct LabelElem<LB_U16>  { typedef unsigned short T; static constexpr int BYTES = 2; };
template <> struct LabelElem<LB_I32>  { typedef int T;            static constexpr int BYTES = 4; };
template <> struct LabelElem<LB_RGB8> { typedef unsigned char T;  static constexpr int BYTES = 3; };

// the rows [i0, i1) of image p, clamped to [0, B): whatever the offsets hold, no row outside the call's planes is written
__device__ inline void label_rows(const int* __restrict__ inst_offsets, int p, int B, int* i0, int* i1) {
  const int a = __builtin_amdgcn_readfirstlane(inst_offsets[p]), b = __builtin_amdgcn_readfirstlane(inst_offsets[p + 1]);
  *i0 = a < 0 ? 0 : a;
  *i1 = b > B ? B : b;
}

__global__ __launch_bounds__(256) void clear_area_kernel(int* __restrict__ area, int B) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i < B) area[i] = 0;
}

// area[b] += popcount over the wave: one vector atomic per wave and instance (none for a wave that holds no pixel of it)
__device__ inline void label_area(int* __restrict__ area, int b, unsigned pat) {
  const int n = wave_sum_i(__popc(pat));
  if (area && n && (threadIdx.x & 63) == 0) atomicAdd(area + b, n);
}

// the 32 labels of an output word, as loaded (2 / 4 / 8 groups of 16 bytes), against one id (wave-uniform), both sides as int32:
// the compare of pack_labels_vec_kernel below, for the frames form (the older kernel keeps its own text - and so the instruction
// stream it had: moved into this function its U16 / I32 loops schedule differently - tried again when this unit was split off: U8
// identical, U16 50 -> 63 VGPRs, I32 another order of the same 385 instructions)
template <int KIND>
__device__ inline unsigned label_word_pattern(const u32x4* q, int id) {
  constexpr int NQ = 2 * LabelElem<KIND>::BYTES;
  unsigned pat = 0;
  if constexpr (KIND == LB_U8) {
    const unsigned s = (unsigned)(id & 255) * 0x01010101u;
    pat = ~(nz16(q[0].x ^ s, q[0].y ^ s, q[0].z ^ s, q[0].w ^ s) | (nz16(q[1].x ^ s, q[1].y ^ s, q[1].z ^ s, q[1].w ^ s) << 16));
    if ((unsigned)id > 255u) pat = 0;
  } else if constexpr (KIND == LB_U16) {
    const unsigned s = (unsigned)(id & 0xffff) * 0x00010001u;
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      const unsigned x[4] = {q[k].x ^ s, q[k].y ^ s, q[k].z ^ s, q[k].w ^ s};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        pat |= ((x[j] & 0xffffu) == 0 ? 1u : 0u) << (8 * k + 2 * j) | ((x[j] >> 16) == 0 ? 1u : 0u) << (8 * k + 2 * j + 1);
    }
    if ((unsigned)id > 65535u) pat = 0;
  } else {
#pragma unroll
    for (int k = 0; k < NQ; ++k)
      pat |= ((int)q[k].x == id ? 1u : 0u) << (4 * k) | ((int)q[k].y == id ? 1u : 0u) << (4 * k + 1) |
             ((int)q[k].z == id ? 1u : 0u) << (4 * k + 2) | ((int)q[k].w == id ? 1u : 0u) << (4 * k + 3);
  }
  return pat;
}

// Vector form (chosen on the host: U8 / U16 / I32, W_out == W, H*W % 32 == 0, every label plane 16-byte aligned): a workgroup owns
// 256 consecutive output words of one image; each lane loads the 32 labels of its word once (2 / 4 / 8 loads of 16 bytes) and
// stores one word per instance - 256 contiguous bytes per wave.  blockIdx.x = image * chunks + chunk.
template <int KIND>
__global__ __launch_bounds__(256) void pack_labels_vec_kernel(const void* __restrict__ labels, long long plane_stride_bytes, int nwords,
                                                              int chunks, const int* __restrict__ inst_offsets,
                                                              const int* __restrict__ inst_label, int B, unsigned* __restrict__ out,
                                                              long long out_stride, int* __restrict__ area) {
  constexpr int NQ = 2 * LabelElem<KIND>::BYTES;   // 16-byte groups per output word
  const int p = blockIdx.x / chunks, chunk = blockIdx.x - p * chunks;
  int i0, i1;
  label_rows(inst_offsets, p, B, &i0, &i1);
  if (i0 >= i1) return;   // (uniform) an image without instances is never read
  const int w = chunk * 256 + (int)threadIdx.x;
  const bool live = w < nwords;
  u32x4 q[NQ];
  const u32x4* s4 = reinterpret_cast<const u32x4*>(static_cast<const unsigned char*>(labels) + (long long)p * plane_stride_bytes) +
                    (long long)w * NQ;
#pragma unroll
  for (int k = 0; k < NQ; ++k) q[k] = live ? __builtin_nontemporal_load(s4 + k) : u32x4{0u, 0u, 0u, 0u};
  unsigned* o = out + w;
  for (int b = i0; b < i1; ++b) {   // uniform trip count: every lane takes part in the reduction
    const int id = inst_label[b];   // (wave-uniform)
    unsigned pat = 0;
    if constexpr (KIND == LB_U8) {
      const unsigned s = (unsigned)(id & 255) * 0x01010101u;
      pat = ~(nz16(q[0].x ^ s, q[0].y ^ s, q[0].z ^ s, q[0].w ^ s) | (nz16(q[1].x ^ s, q[1].y ^ s, q[1].z ^ s, q[1].w ^ s) << 16));
      if ((unsigned)id > 255u) pat = 0;
    } else if constexpr (KIND == LB_U16) {
      const unsigned s = (unsigned)(id & 0xffff) * 0x00010001u;
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        const unsigned x[4] = {q[k].x ^ s, q[k].y ^ s, q[k].z ^ s, q[k].w ^ s};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          pat |= ((x[j] & 0xffffu) == 0 ? 1u : 0u) << (8 * k + 2 * j) | ((x[j] >> 16) == 0 ? 1u : 0u) << (8 * k + 2 * j + 1);
      }
      if ((unsigned)id > 65535u) pat = 0;
    } else {
#pragma unroll
      for (int k = 0; k < NQ; ++k)
        pat |= ((int)q[k].x == id ? 1u : 0u) << (4 * k) | ((int)q[k].y == id ? 1u : 0u) << (4 * k + 1) |
               ((int)q[k].z == id ? 1u : 0u) << (4 * k + 2) | ((int)q[k].w == id ? 1u : 0u) << (4 * k + 3);
    }
    if (!live) pat = 0;
    if (live) o[(long long)b * out_stride] = pat;
    label_area(area, b, pat);
  }
}

// General form: one thread per output word, any stride / alignment / row padding, a ragged last word, RGB8; element (v, u) is read
// when v < H and u < W, zero-extended (RGB8: R + 256 G + 65536 B).
template <int KIND>
__global__ __launch_bounds__(256) void pack_labels_kernel(const void* __restrict__ labels, long long plane_stride_elems, int H, int W,
                                                          int W_out, int nwords, int chunks, const int* __restrict__ inst_offsets,
                                                          const int* __restrict__ inst_label, int B, unsigned* __restrict__ out,
                                                          long long out_stride, int* __restrict__ area) {
  typedef typename LabelElem<KIND>::T T;
  const int p = blockIdx.x / chunks, chunk = blockIdx.x - p * chunks;
  int i0, i1;
  label_rows(inst_offsets, p, B, &i0, &i1);
  if (i0 >= i1) return;   // (uniform)
  const int w = chunk * 256 + (int)threadIdx.x;
  const bool live = w < nwords;
  const T* sp = static_cast<const T*>(labels) + (long long)p * plane_stride_elems * (KIND == LB_RGB8 ? 3 : 1);
  const long long total = (long long)H * W_out, j0 = (long long)w * 32;
  int v = (int)(j0 / W_out), u = (int)(j0 - (long long)v * W_out);
  int lab[32];
  unsigned have = 0;   // bit k: pixel k of the word lies inside the image
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    lab[k] = 0;
    if (live && j0 + k < total && u < W) {
      const long long e = (long long)v * W + u;
      if constexpr (KIND == LB_RGB8) lab[k] = (int)sp[e * 3] | (int)sp[e * 3 + 1] << 8 | (int)sp[e * 3 + 2] << 16;
      else lab[k] = (int)sp[e];
      have |= 1u << k;
    }
    if (++u == W_out) { u = 0; ++v; }
  }
  unsigned* o = out + w;
  for (int b = i0; b < i1; ++b) {   // uniform trip count
    const int id = inst_label[b];
    unsigned pat = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) pat |= (lab[k] == id ? 1u : 0u) << k;
    pat &= have;
    if (live) o[(long long)b * out_stride] = pat;
    label_area(area, b, pat);
  }
}

// ---- label maps of images of different sizes (la3d_pack_label_bits_frames) -------------------
// The two forms above with the geometry of every image read from its la3d_frame row (wave-uniform: scalar loads) and the plane of
// every (image, id) row at its own offset.  The pitch of a conforming row is a multiple of 32, so a word never straddles two rows:
// word w of an image holds columns 32 (w % (W/32)) .. + 31 of row w / (W/32), and `have` clears the bits of the columns >=
// frame_width whatever the padding elements hold.  A row that breaks the contract (frame_row_ok: the check the fit makes) is left
// before anything is read through it; so is a plane whose offset is negative or not a multiple of 4 (frames_prologue, frames_plane_at).
// blockIdx.x = image * chunks + chunk, chunks sized for the bounds' plane: a chunk beyond its image's words returns before any load.

// U8 / U16 / I32: each lane loads the 32 labels of its word once - in 16-byte groups where the plane is 16-byte aligned (labels is, and
// depth_offset % 4 == 0 makes every I32 plane so; a U8 / U16 plane whose offset is not a multiple of 16 / 8 elements takes the same
// bytes in 4-byte loads) - and stores one word per instance
template <int KIND>
__global__ __launch_bounds__(256) void pack_labels_frames_vec_kernel(const void* __restrict__ labels, const la3d_frame* __restrict__ frames,
                                                                     int max_h, int max_w, int chunks, const int* __restrict__ inst_offsets,
                                                                     const int* __restrict__ inst_label, int B, unsigned* __restrict__ out,
                                                                     const long long* __restrict__ out_offsets, int* __restrict__ area) {
  constexpr int NQ = 2 * LabelElem<KIND>::BYTES;   // 16-byte groups per output word
  const int p = blockIdx.x / chunks, chunk = blockIdx.x - p * chunks;
  int i0, i1;
  label_rows(inst_offsets, p, B, &i0, &i1);
  if (i0 >= i1) return;   // (uniform) an image without instances is never read
  FramesWork f;
  if (!frames_prologue<false, true>(frames, 0, nullptr, max_h, max_w, nullptr, nullptr, p, chunk, &f)) return;   // (uniform)
  const FrameRow& r = f.r;
  const int w = f.w;
  const bool live = f.live;
  const unsigned have = f.have;
  const long long base_bytes = r.off * LabelElem<KIND>::BYTES;
  const unsigned char* plane = static_cast<const unsigned char*>(labels) + base_bytes;
  u32x4 q[NQ];
  if ((base_bytes & 15) == 0) {   // uniform
    const u32x4* s4 = reinterpret_cast<const u32x4*>(plane) + (long long)w * NQ;
#pragma unroll
    for (int k = 0; k < NQ; ++k) q[k] = live ? __builtin_nontemporal_load(s4 + k) : u32x4{0u, 0u, 0u, 0u};
  } else {
    const unsigned* s1 = reinterpret_cast<const unsigned*>(plane) + (long long)w * NQ * 4;
#pragma unroll
    for (int k = 0; k < NQ; ++k) q[k] = live ? u32x4{s1[4 * k], s1[4 * k + 1], s1[4 * k + 2], s1[4 * k + 3]} : u32x4{0u, 0u, 0u, 0u};
  }
  for (int b = i0; b < i1; ++b) {   // uniform trip count: every lane takes part in the reduction
    long long oo;
    if (!frames_plane_at(out_offsets, b, &oo)) continue;   // (uniform) the fit refuses this instance too
    const int id = inst_label[b];   // (wave-uniform)
    const unsigned pat = label_word_pattern<KIND>(q, id) & have;
    if (live) out[oo + w] = pat;
    label_area(area, b, pat);
  }
}

// RGB8 (3 bytes per pixel: no 16-byte form): one thread per output word, the image columns of its 32 pixels read byte by byte
__global__ __launch_bounds__(256) void pack_labels_frames_rgb8_kernel(const unsigned char* __restrict__ labels, const la3d_frame* __restrict__ frames,
                                                                      int max_h, int max_w, int chunks, const int* __restrict__ inst_offsets,
                                                                      const int* __restrict__ inst_label, int B, unsigned* __restrict__ out,
                                                                      const long long* __restrict__ out_offsets, int* __restrict__ area) {
  const int p = blockIdx.x / chunks, chunk = blockIdx.x - p * chunks;
  int i0, i1;
  label_rows(inst_offsets, p, B, &i0, &i1);
  if (i0 >= i1) return;   // (uniform)
  FramesWork f;
  if (!frames_prologue<false, true>(frames, 0, nullptr, max_h, max_w, nullptr, nullptr, p, chunk, &f)) return;   // (uniform)
  const FrameRow& r = f.r;
  const int w = f.w;
  const bool live = f.live;
  const unsigned have = f.have;
  const unsigned char* sp = labels + (r.off + (long long)w * 32) * 3;   // (pixel 32 w of the plane: row w / (W/32), column 32 (w % (W/32)))
  int lab[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    lab[k] = 0;
    if ((have >> k) & 1u) lab[k] = (int)sp[k * 3] | (int)sp[k * 3 + 1] << 8 | (int)sp[k * 3 + 2] << 16;
  }
  for (int b = i0; b < i1; ++b) {   // uniform trip count
    long long oo;
    if (!frames_plane_at(out_offsets, b, &oo)) continue;   // (uniform)
    const int id = inst_label[b];
    unsigned pat = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) pat |= (lab[k] == id ? 1u : 0u) << k;
    pat &= have;
    if (live) out[oo + w] = pat;
    label_area(area, b, pat);
  }
}

// ---- u8 masks and logits of images of different sizes (la3d_pack_mask_bits_frames / la3d_pack_logits_bits_frames) ------------
// One plane per INSTANCE, each of its own image's size, anywhere behind one base pointer: what an instance-segmentation network
// hands over per image, read where it lies.  One lane per output word, blockIdx.x = instance * chunks + chunk, chunks sized for the
// bounds' plane.  Everything that decides whether and where something is read or written is wave-uniform (scalar loads) and checked
// BEFORE an address is formed from it, in this order:
//   image_index outside [0, P), a frame row that breaks the contract (frame_row_ok: the check the fit makes), a bits_offsets entry
//   that is negative or no multiple of 4: return - nothing read, nothing written, area stays 0 (the fit gives these status 5);
//   a chunk beyond the instance's words: return before any load;
//   a negative src_offsets entry or a pitch < frame_width: the plane is written as zeros, nothing is read (status 1 in the fit).
// What is read of a conforming instance: elements (v, u) with v < H and u < pitch; in the last row none with u >= frame_width.
//   16-byte form (the plane's first byte and its byte pitch are multiples of 16; a word starts 32 elements = a multiple of 16 bytes
//   into its row, so every group address is 16-byte aligned): a group is loaded whole only if its first column cg < frame_width.  The
//   pitch is then a multiple of the group's EPG elements, as cg is, so cg < frame_width <= pitch gives cg + EPG <= pitch: the group lies
//   inside row v.  In the LAST row a group is loaded whole only if cg + EPG <= frame_width; one that reaches past it takes the
//   element form, so nothing behind the last image column of the last row is touched (a dense plane may end its allocation).
//   Element form (everything else): element (v, u) is loaded only where u < frame_width <= pitch.
// The bits of columns >= frame_width are cleared by image_columns() whatever a whole group brought along.
template <int KIND>
__global__ __launch_bounds__(256) void pack_masks_frames_kernel(const void* __restrict__ src, const la3d_frame* __restrict__ frames, int P,
                                                                int max_h, int max_w, int chunks, const int* __restrict__ image_index,
                                                                const long long* __restrict__ src_offsets, const int* __restrict__ src_pitch,
                                                                float thr, unsigned* __restrict__ out,
                                                                const long long* __restrict__ out_offsets, int* __restrict__ area) {
  typedef typename PackElem<KIND>::T T;
  constexpr int ES = (int)sizeof(T);
  constexpr int EPG = 16 / ES;    // elements per 16-byte group: 16 / 8 / 4
  constexpr int NQ = 32 / EPG;    // groups per output word: 2 / 4 / 8
  const int n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
  FramesWork f;
  if (!frames_prologue<true, true>(frames, P, image_index, max_h, max_w, out, out_offsets, n, chunk, &f)) return;   // (uniform) nothing read or written
  const FrameRow& r = f.r;
  const long long oo = f.off;
  const int w = f.w;
  const bool live = f.live;
  const long long so = uniform_i64(src_offsets[n]);
  const int pitch = src_pitch ? __builtin_amdgcn_readfirstlane(src_pitch[n]) : r.fw;
  if (so < 0 || pitch < r.fw) {   // (uniform) a source that cannot be read: an empty plane, never what the memory held before
    if (live) out[oo + w] = 0u;
    return;
  }
  unsigned pat = 0;
  if (live) {
    const int wpr = r.W >> 5;
    const int v = w / wpr, c0 = (w - v * wpr) << 5;   // row and first column of this word
    const T* sp = static_cast<const T*>(src) + so + (long long)v * pitch + c0;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) + (unsigned long long)so * ES) & 15) == 0 && (((long long)pitch * ES) & 15) == 0;   // uniform
    const bool last = v == r.H - 1;
#pragma unroll
    for (int g = 0; g < NQ; ++g) {
      const int cg = c0 + g * EPG;
      unsigned gb = 0;
      if (vec && cg < r.fw && (!last || cg + EPG <= r.fw)) {
        gb = pack_group<KIND>(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(sp + g * EPG)), thr);
      } else {
#pragma unroll
        for (int e = 0; e < EPG; ++e)
          if (cg + e < r.fw && pack_pred<KIND>(sp[g * EPG + e], thr)) gb |= 1u << e;
      }
      pat |= gb << (g * EPG);
    }
    pat &= image_columns(w, r.W, r.fw);   // (= f.have, formed here: held from the prologue it costs two more VGPRs)
    out[oo + w] = pat;
  }
  label_area(area, n, pat);   // (every lane of the wave takes part)
}

// ---- crop-space masks -> bit planes (la3d_pack_crop_bits / la3d_pack_crop_bits_frames) ------------------------------------------
// restore_mask_from_crop for a batch (reference src/util.py:171-214, called at src/batch_scripts/whole.py:94): the S x S crop of
// instance n, resized by nearest index to side x side pixels and pasted at (x1, y1), clipped to the frame - written as the plane's
// words, never as a u8 plane.  One lane per output word, blockIdx.x = instance, blockIdx.y = chunk of 256 words (sized for the bounds'
// plane in the frames form: a chunk beyond its plane returns before any load).  A word is 32 independent source lookups; where the
// stored rows are whole words (W % 32 == 0) a word lies in one frame row and so in one source row, and a word whose row or columns
// miss the placement is stored as zero without a load.
// What decides whether and where something is read: the row of `place` - wave-uniform, through scalar loads, checked BEFORE an address
// is formed from it.
//   side outside (0, CROP_SIDE_MAX], or a placement that misses the frame (x1 >= frame_width, x1 + side <= 0, y1 >= H, y1 + side <= 0,
//   in 64 bits: x1, y1 are any int32): nothing is read, the plane is zero.
//   Otherwise the 32 lookups of a word that meets the placement are issued TOGETHER, each at a distance d CLAMPED into [0, side - 1]
//   (a bit whose own pixel misses the placement looks up the nearest one that does not, and is masked out afterwards): the loads do
//   not wait for one another.  0 <= d < 2^20 is exact in float64 and ifx > 0, so 0 <= min(floor(d * ifx), S - 1) <= S - 1: only bytes
//   (y, x) in [0, S)^2 of the instance's OWN crop are ever addressed, whatever place holds.
constexpr int CROP_SIDE_MAX = 1 << 20;
struct CropSrc {
  const unsigned char* crops;   // byte (y, x) of crop n at crops + n * stride + y * pitch + x * step
  long long stride;
  int pitch, step, S, thr;      // bit = byte > thr
  const int* place;             // dev [B][4]: x1, y1, side, 0
};

// OpenCV's resizeNN index rule (inv_scale = dsize / ssize, ifx = 1 / inv_scale): min(floor(d * ifx), S - 1).  The product is ONE
// float64 multiply, rounded on its own (__dmul_rn: never contracted with anything around it), then floor.  d is clamped into
// [0, side - 1] first: `in` tells whether it was inside.
__device__ inline int crop_index(long long d, int side, double ifx, int S, bool* in) {
  *in = d >= 0 && d < side;
  const int dc = d < 0 ? 0 : d < side ? (int)d : side - 1;
  const int i = (int)floor(__dmul_rn((double)dc, ifx));
  return i < S - 1 ? i : S - 1;
}

template <bool FRAMES>
__global__ __launch_bounds__(256) void pack_crop_bits_kernel(const CropSrc s, const BitsOut c) {
  const int n = blockIdx.x, chunk = blockIdx.y;
  PlaneGeo g;
  if (!plane_geometry<FRAMES>(c, n, &g)) return;   // (uniform) refused: no plane word, the area stays 0
  if (chunk * 256 >= g.nwords) return;             // (uniform) before any load
  const int w = chunk * 256 + (int)threadIdx.x;
  const bool live = w < g.nwords;
  const int fw = g.fw > 0 ? g.fw : g.W;            // the image columns
  const int* pl = s.place + (long long)n * 4;
  const int x1 = __builtin_amdgcn_readfirstlane(pl[0]), y1 = __builtin_amdgcn_readfirstlane(pl[1]);
  const int side = __builtin_amdgcn_readfirstlane(pl[2]);
  const bool shows = side > 0 && side <= CROP_SIDE_MAX && x1 < fw && (long long)x1 + side > 0 && y1 < g.H && (long long)y1 + side > 0;   // uniform
  unsigned pat = 0;
  if (live && shows) {
    const double ifx = 1.0 / ((double)side / (double)s.S);
    const unsigned char* crop = s.crops + (long long)n * s.stride;
    bool in;
    if ((g.W & 31) == 0) {   // uniform: a word lies in one row
      const int wpr = g.W >> 5;
      const int v = w / wpr, c0 = (w - v * wpr) << 5;
      const long long dx0 = (long long)c0 - x1;
      const int sy = crop_index((long long)v - y1, side, ifx, s.S, &in);   // (v < H: w < nwords)
      if (in && dx0 + 31 >= 0 && dx0 < side) {
        const unsigned char* row = crop + (long long)sy * s.pitch;
        unsigned have = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
          const int sx = crop_index(dx0 + k, side, ifx, s.S, &in);
          have |= (in && c0 + k < fw ? 1u : 0u) << k;
          pat |= ((int)row[(long long)sx * s.step] > s.thr ? 1u : 0u) << k;
        }
        pat &= have;
      }
    } else {                 // W_out == W, no multiple of 32: a word may straddle rows - bit by bit
      const long long total = (long long)g.H * g.W, i0 = (long long)w * 32;
      const long long last = i0 + 31 < total ? i0 + 31 : total - 1;
      int v = (int)(i0 / g.W), u = (int)(i0 - (long long)v * g.W);
      if (last / g.W >= y1 && v < (long long)y1 + side) {   // one of the word's rows meets the placement
        unsigned have = 0;
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
          bool iny;
          const int sy = crop_index((long long)v - y1, side, ifx, s.S, &iny), sx = crop_index((long long)u - x1, side, ifx, s.S, &in);
          have |= (in && iny && u < fw && i0 + k < total ? 1u : 0u) << k;
          pat |= ((int)crop[(long long)sy * s.pitch + (long long)sx * s.step] > s.thr ? 1u : 0u) << k;
          if (++u == g.W) { u = 0; ++v; }
        }
        pat &= have;
      }
    }
  }
  if (live) g.out[w] = pat;
  label_area(c.area, n, pat);   // (every lane of the wave takes part)
}

}  // namespace

// ==========================================================================================
// host side: the destination, the ONE argument check and the launch helpers of the packer entries
// ==========================================================================================
namespace {
// workgroups per plane: enough to cover `items` once, at most 64 (grid-stride inside the plane beyond that)
inline int plane_chunks(long long items) {
  const long long c = (items + 255) / 256;
  return (int)(c < 1 ? 1 : (c > 64 ? 64 : c));
}

const char* const SIZES_UNIFORM = "bad argument (B >= 0, H, W > 0, W_out >= W)";
const char* const BITS_4 = "bits not a 4-byte aligned pointer";
const char* const LABEL_DTYPE = "unknown dtype (LA3D_LABEL_U8, LA3D_LABEL_U16, LA3D_LABEL_I32 or LA3D_LABEL_RGB8)";
const char* const LABEL_PTRS_4 = "inst_offsets, inst_label or area not a 4-byte aligned pointer";

// area (may be NULL) cleared by a kernel of the call's own on the call's stream - a kernel node like the packer's when captured - and
// the launch checked
int clear_area(int32_t* area, int B, hipStream_t s) {
  if (!area) return LA3D_SUCCESS;
  hipLaunchKernelGGL(clear_area_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, area, B);
  return check_launch("clear_area_kernel");
}

// a runtime element kind (PK_* / LB_*: 0 .. 3, checked by the entry) -> a template argument: f(std::integral_constant<int, KIND>())
template <typename F>
int with_kind(int kind, F&& f) {
  switch (kind) {
    case 0: return f(std::integral_constant<int, 0>());
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    default: return f(std::integral_constant<int, 3>());
  }
}
inline unsigned pack_elem_mask(int kind) { return kind == PK_F32 ? 3u : kind == PK_U8 ? 0u : 1u; }   // alignment of a source element

template <int KIND>
int pack_bits_launch(const void* src, long long plane_stride, float thr, int B, int H, int W, int W_out, uint32_t* bits,
                     long long bits_plane_stride, hipStream_t s, const char* what) {
  constexpr long long ES = (long long)sizeof(typename PackElem<KIND>::T);
  const long long HW = (long long)H * W;
  const int nwords = (int)la3d_mask_bits_words(H, W_out);
  // (CallFacts::vec of the packers: one linear run of whole words per plane, every plane base 16-byte aligned)
  const bool vec = W_out == W && HW % 32 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (plane_stride * ES) % 16 == 0;
  if (vec) {
    const int chunks = plane_chunks(HW / (16 / ES));
    hipLaunchKernelGGL(pack_bits_vec_kernel<KIND>, dim3((unsigned)((long long)B * chunks)), dim3(256), 0, s, src, plane_stride * ES, thr, (int)HW,
                       chunks, bits, bits_plane_stride);
  } else {
    const int chunks = plane_chunks(nwords);
    hipLaunchKernelGGL(pack_bits_kernel<KIND>, dim3((unsigned)((long long)B * chunks)), dim3(256), 0, s, src, plane_stride, thr, H, W, W_out,
                       nwords, chunks, bits, bits_plane_stride);
  }
  return check_launch(what);
}

// the check and the launch la3d_pack_mask_bits / la3d_pack_logits_bits share; kind: PK_*
int pack_bits(const char* who, const char* kernel, const void* src, int kind, long long plane_stride, float thr, int B, int H, int W, int W_out,
              uint32_t* bits, long long bits_plane_stride, void* stream) {
  static const char* const nb = "NULL input or bits not a 4-byte aligned pointer";
  static const PackWords say = {SIZES_UNIFORM, "frame or batch too large (H*W_out <= 2^28, B <= 2^25)", nb, nullptr,
                                "input plane stride smaller than H*W", BITS_STRIDE};
  const int rc = pack_check(who, say, B, 1, W, B > 0, plane_items(H, W_out) > (1LL << 28) || (long long)B * 64 > 0x7fffffffLL, false,
                            {{src, 0, nb}, {bits, 3, nb}}, plane_stride, bits_out_uniform(H, W, W_out, bits, bits_plane_stride, nullptr));
  if (rc != PACK_LAUNCH) return pack_done(rc);
  return with_kind(kind, [&](auto k) {
    return pack_bits_launch<decltype(k)::value>(src, plane_stride, thr, B, H, W, W_out, bits, bits_plane_stride, static_cast<hipStream_t>(stream), kernel);
  });
}

// ---- annotations -> bit planes: the check of either form (s0, s1, s2: the annotation arrays; run lengths have two) and what the
// four entries share behind it.  The LDS rule ranks in front of the stride rule: the stride's word count is then known to fit an int.
int ann_check(const char* who, const void* s0, const void* s1, const void* s2, int B, int W, const BitsOut& c) {
  static const char* const a4 = "bits or area not a 4-byte aligned pointer";
  static const PackWords say = {SIZES_UNIFORM, "W_out must be W or a multiple of 32 (padded rows are whole words)", "NULL annotation arrays or bits",
                                "the bit image must fit LDS (H*W_out <= 1048576)", nullptr, BITS_STRIDE};
  return pack_check(who, say, B, 1, W, B > 0, c.W != W && c.W % 32 != 0, plane_items(c.H, c.W) > (1LL << 20),
                    {{s0, 0, nullptr}, {s1, 0, nullptr}, {s2, 0, nullptr}, {c.bits, 3, a4}, {c.area, 3, a4, true}}, 0, c);
}
int ann_frames_check(const char* who, const void* s0, const void* s1, const void* s2, int B, const BitsOut& c) {
  static const char* const p8 = "frames or bits_offsets not an 8-byte aligned pointer";
  static const char* const p4 = "image_index or area not a 4-byte aligned pointer";
  static const PackWords say = {SIZES_FRAMES, nullptr, "NULL annotation arrays, frames, image_index, bits or bits_offsets",
                                "the bit image of the bounds must fit LDS (H * roundup32(W) <= 1048576)", nullptr, nullptr};
  return pack_check(who, say, B, c.P, c.W, B > 0, false, bounds_words(c.H, c.W) > (1LL << 15),
                    {{s0, 0, nullptr}, {s1, 0, nullptr}, {s2, 0, nullptr}, {c.bits, 15, "bits not a 16-byte aligned pointer"},
                     {c.frames, 7, p8, c.P == 0}, {c.offsets, 7, p8}, {c.image_index, 3, p4}, {c.area, 3, p4, true}}, 0, c);
}
inline size_t rle_bits_lds(int lds_words, int scan_words) { return (size_t)lds_words * 4 + 64 + (size_t)scan_words * 4; }
inline size_t poly_bits_lds(int lds_words) { return (((size_t)lds_words * 4 + 15) & ~(size_t)15) + POLY_STAGE_BYTES + 64; }

template <bool FRAMES>
int pack_rle_launch(const char* who, const char* kernel, const int32_t* counts, const int64_t* offsets, int B, int scan_words, const BitsOut& c,
                    void* stream) {
  const size_t lds = rle_bits_lds(c.lds_words, scan_words);
  if (lds > ANN_LDS_MAX) return refuse(who, "frame too large for LDS", LA3D_ERR_UNSUPPORTED);
  allow_big_lds(reinterpret_cast<const void*>(pack_rle_bits_kernel<FRAMES>));
  hipLaunchKernelGGL(pack_rle_bits_kernel<FRAMES>, dim3(B), dim3(NT_DEC), lds, static_cast<hipStream_t>(stream), counts,
                     reinterpret_cast<const long long*>(offsets), scan_words, c);
  return check_launch(kernel);
}
template <bool FRAMES>
int pack_poly_launch(const char* who, const char* kernel, const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, int B,
                     const BitsOut& c, void* stream) {
  const size_t lds = poly_bits_lds(c.lds_words);
  if (lds > ANN_LDS_MAX) return refuse(who, "frame too large for LDS", LA3D_ERR_UNSUPPORTED);
  allow_big_lds(reinterpret_cast<const void*>(pack_poly_bits_kernel<FRAMES>));
  hipLaunchKernelGGL(pack_poly_bits_kernel<FRAMES>, dim3(B), dim3(NT_DEC), lds, static_cast<hipStream_t>(stream), poly_xy,
                     reinterpret_cast<const long long*>(ring_offsets), reinterpret_cast<const long long*>(inst_rings), c);
  return check_launch(kernel);
}

// ---- label maps ----
template <int KIND>
int pack_labels_launch(const void* labels, long long plane_stride, int P, int H, int W, int W_out, const int* inst_offsets,
                       const int* inst_label, int B, uint32_t* bits, long long bits_plane_stride, int* area, hipStream_t s) {
  constexpr long long ES = LabelElem<KIND>::BYTES;
  const long long HW = (long long)H * W;
  const int nwords = (int)la3d_mask_bits_words(H, W_out);
  const int chunks = (nwords + 255) / 256;
  const bool vec = KIND != LB_RGB8 && W_out == W && HW % 32 == 0 && (reinterpret_cast<uintptr_t>(labels) & 15) == 0 &&
                   (plane_stride * ES) % 16 == 0;
  const dim3 grid((unsigned)((long long)P * chunks));
  if constexpr (KIND != LB_RGB8) {
    if (vec) {
      hipLaunchKernelGGL(pack_labels_vec_kernel<KIND>, grid, dim3(256), 0, s, labels, plane_stride * ES, nwords, chunks, inst_offsets,
                         inst_label, B, bits, bits_plane_stride, area);
      return check_launch("pack_labels_vec_kernel");
    }
  }
  hipLaunchKernelGGL(pack_labels_kernel<KIND>, grid, dim3(256), 0, s, labels, plane_stride, H, W, W_out, nwords, chunks, inst_offsets,
                     inst_label, B, bits, bits_plane_stride, area);
  return check_launch("pack_labels_kernel");
}

template <int KIND>
int pack_labels_frames_launch(const void* labels, int chunks, const int* inst_offsets, const int* inst_label, int B, const BitsOut& c,
                              hipStream_t s) {
  const dim3 grid((unsigned)((long long)c.P * chunks));
  if constexpr (KIND == LB_RGB8)
    hipLaunchKernelGGL(pack_labels_frames_rgb8_kernel, grid, dim3(256), 0, s, static_cast<const unsigned char*>(labels), c.frames, c.H, c.W, chunks,
                       inst_offsets, inst_label, B, c.bits, c.offsets, c.area);
  else
    hipLaunchKernelGGL(pack_labels_frames_vec_kernel<KIND>, grid, dim3(256), 0, s, labels, c.frames, c.H, c.W, chunks, inst_offsets, inst_label, B,
                       c.bits, c.offsets, c.area);
  return check_launch("pack_labels_frames_kernel");
}

// ---- u8 masks and logits of images of different sizes: the check and the launch the two entries share; kind: PK_* ----
int pack_masks_frames(const char* who, const void* src, int kind, float thr, const la3d_frame* frames, int P, int H, int W,
                      const int32_t* image_index, const int64_t* src_offsets, const int32_t* src_pitch, int B, uint32_t* bits,
                      const int64_t* bits_offsets, int32_t* area, void* stream) {
  static const char* const p8 = "frames, src_offsets or bits_offsets not an 8-byte aligned pointer";
  static const char* const p4 = "image_index, src_pitch or area not a 4-byte aligned pointer";
  static const PackWords say = {SIZES_FRAMES, "bounds or batch too large (H * roundup32(W) <= 2^28, B * ceil(H * roundup32(W) / 8192) < 2^31)",
                                "NULL source, frames, image_index, src_offsets, bits or bits_offsets", nullptr, nullptr, nullptr};
  const BitsOut c = bits_out_frames(frames, P, H, W, image_index, bits, bits_offsets, area);
  const long long words = bounds_words(H, W), chunks = (words + 255) / 256;
  const int rc = pack_check(who, say, B, P, W, B > 0 && P > 0, words > (1LL << 23) || (long long)B * chunks > 0x7fffffffLL, false,
                            {{src, pack_elem_mask(kind), "source not aligned to its element size"}, {bits, 3, BITS_4}, {frames, 7, p8},
                             {src_offsets, 7, p8}, {bits_offsets, 7, p8}, {image_index, 3, p4}, {src_pitch, 3, p4, true}, {area, 3, p4, true}}, 0, c);
  if (rc != PACK_LAUNCH) return pack_done(rc);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cleared = clear_area(area, B, s);
  if (cleared != LA3D_SUCCESS) return cleared;
  return with_kind(kind, [&](auto k) {
    hipLaunchKernelGGL(pack_masks_frames_kernel<decltype(k)::value>, dim3((unsigned)((long long)B * chunks)), dim3(256), 0, s, src, frames, P, H, W,
                       (int)chunks, image_index, reinterpret_cast<const long long*>(src_offsets), src_pitch, thr, bits, c.offsets, area);
    return check_launch("pack_masks_frames_kernel");
  });
}

// ---- crop-space masks: the rules of the source (either form, in front of the packers' check) and the launch behind it ----
int crop_source(const char* who, const uint8_t* crops, int64_t crop_stride, int32_t row_pitch, int32_t pixel_step, int S, int threshold,
                const int32_t* place, int B, CropSrc* s) {
  if (S <= 0 || pixel_step < 1 || (long long)row_pitch < (long long)S * pixel_step || threshold < 0 || threshold > 255)
    return refuse(who, "bad source (S > 0, pixel_step >= 1, row_pitch >= S * pixel_step, 0 <= threshold <= 255)");
  // (the bytes of one crop: its last row ends S * pixel_step - (pixel_step - 1) bytes in)
  if (crop_stride < (long long)(S - 1) * row_pitch + (long long)(S - 1) * pixel_step + 1 || (B > 0 && crop_stride > INT64_MAX / B))
    return refuse(who, "crop_stride is smaller than a crop (or B * crop_stride overflows)");
  if (B > 0 && (reinterpret_cast<uintptr_t>(place) & 3)) return refuse(who, "place not a 4-byte aligned pointer");
  *s = CropSrc{crops, (long long)crop_stride, row_pitch, pixel_step, S, threshold, place};
  return LA3D_SUCCESS;
}
template <bool FRAMES>
int pack_crop_launch(const CropSrc& src, int B, const BitsOut& c, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cleared = clear_area(c.area, B, s);
  if (cleared != LA3D_SUCCESS) return cleared;
  hipLaunchKernelGGL(pack_crop_bits_kernel<FRAMES>, dim3((unsigned)B, (unsigned)((c.lds_words + 255) / 256)), dim3(256), 0, s, src, c);
  return check_launch("pack_crop_bits_kernel");
}
}  // namespace

extern "C" {

int la3d_rle_decode(const int32_t* counts, const int64_t* offsets, int B, int H, int W, uint8_t* mask_out, void* stream) {
  if ((!counts && B > 0) || !offsets || !mask_out || B < 0 || H <= 0 || W <= 0 || (long long)H * W > (1LL << 20))
    return refuse("la3d_rle_decode", "bad argument (H*W <= 1048576)");
  if (B == 0) return LA3D_SUCCESS;
  const int nwords = (H * W + 31) / 32;
  // behind the bit image: 16 words of wave totals, then the block totals of the column scan (word-aligned rows)
  const int scan_words = (W % 32 == 0) ? ((NT_DEC / (W / 32) > 2 ? NT_DEC / (W / 32) : 2) * (W / 32)) : 0;
  const size_t lds = (size_t)nwords * 4 + 64 + (size_t)scan_words * 4;
  if (lds > 160 * 1024 - 256) return refuse("la3d_rle_decode", "frame too large for LDS", LA3D_ERR_UNSUPPORTED);
  allow_big_lds(reinterpret_cast<const void*>(rle_decode_kernel));
  hipLaunchKernelGGL(rle_decode_kernel, dim3(B), dim3(NT_DEC), lds, static_cast<hipStream_t>(stream), counts,
                     reinterpret_cast<const long long*>(offsets), H, W, nwords, scan_words, mask_out);
  return check_launch("rle_decode_kernel");
}

int la3d_poly_decode(const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, int B, int H, int W,
                     uint8_t* mask_out, void* stream) {
  if (((!poly_xy || !ring_offsets || !inst_rings || !mask_out) && B > 0) || B < 0 || H <= 0 || W <= 0 ||
      (long long)H * W > (1LL << 20))
    return refuse("la3d_poly_decode", "bad argument (H*W <= 1048576)");
  if (B == 0) return LA3D_SUCCESS;
  const int nwords = (H * W + 31) / 32;
  const size_t lds = (((size_t)nwords * 4 + 15) & ~(size_t)15) + POLY_STAGE_BYTES + 64;
  allow_big_lds(reinterpret_cast<const void*>(poly_decode_kernel));
  hipLaunchKernelGGL(poly_decode_kernel, dim3(B), dim3(NT_DEC), lds, static_cast<hipStream_t>(stream), poly_xy,
                     reinterpret_cast<const long long*>(ring_offsets), reinterpret_cast<const long long*>(inst_rings), H, W, nwords,
                     mask_out);
  return check_launch("poly_decode_kernel");
}

int la3d_pack_mask_bits(const uint8_t* mask, int64_t mask_plane_stride, int B, int H, int W, int W_out, uint32_t* bits,
                        int64_t bits_plane_stride, void* stream) {
  return pack_bits("la3d_pack_mask_bits", "pack_mask_bits_kernel", mask, PK_U8, mask_plane_stride, 0.0f, B, H, W, W_out, bits, bits_plane_stride,
                   stream);
}

int la3d_pack_logits_bits(const void* logits, int dtype, int64_t plane_stride, float threshold, int B, int H, int W, int W_out,
                          uint32_t* bits, int64_t bits_plane_stride, void* stream) {
  const char* who = "la3d_pack_logits_bits";
  if (dtype != LA3D_DTYPE_F32 && dtype != LA3D_DTYPE_F16 && dtype != LA3D_DTYPE_BF16)
    return refuse(who, "unknown dtype (LA3D_DTYPE_F32, LA3D_DTYPE_F16 or LA3D_DTYPE_BF16)");
  const int kind = dtype == LA3D_DTYPE_F32 ? PK_F32 : dtype == LA3D_DTYPE_F16 ? PK_F16 : PK_BF16;
  // (this entry alone ranks the source's alignment in front of the size rules)
  if (B > 0 && (reinterpret_cast<uintptr_t>(logits) & pack_elem_mask(kind))) return refuse(who, "logits not aligned to their element size");
  return pack_bits(who, "pack_logits_bits_kernel", logits, kind, plane_stride, threshold, B, H, W, W_out, bits, bits_plane_stride, stream);
}

int la3d_unpack_mask_bits(const uint32_t* bits, int64_t bits_plane_stride, int B, int H, int W_in, int W, uint8_t* mask, void* stream) {
  if (B < 0 || H <= 0 || W <= 0 || W_in < W || (long long)H * W_in > (1LL << 28) || (long long)B * 64 > 0x7fffffffLL ||
      (B > 0 && (!bits || !mask || (reinterpret_cast<uintptr_t>(bits) & 3) || bits_plane_stride < (int64_t)la3d_mask_bits_words(H, W_in))))
    return refuse("la3d_unpack_mask_bits", "bad argument (W <= W_in, bits 4-byte aligned, bits_plane_stride >= la3d_mask_bits_words(H, W_in))");
  if (B == 0) return LA3D_SUCCESS;
  const int quads = (W % 4 == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0) ? 1 : 0;
  const int chunks = plane_chunks(quads ? (long long)H * W / 4 : (long long)H * W);
  hipLaunchKernelGGL(unpack_mask_bits_kernel, dim3((unsigned)((long long)B * chunks)), dim3(256), 0, static_cast<hipStream_t>(stream), bits,
                     (long long)bits_plane_stride, H, W_in, W, quads, chunks, mask);
  return check_launch("unpack_mask_bits_kernel");
}

int la3d_mask_stats_bits(const uint32_t* bits, int64_t bits_plane_stride, int B, int H, int W, int frame_width, int boundary,
                         int32_t* stats, void* stream) {
  if (B < 0 || H <= 0 || W <= 0 || boundary < 0 || frame_width < 0 || frame_width > W ||
      (B > 0 && (!bits || !stats || (reinterpret_cast<uintptr_t>(bits) & 3) || bits_plane_stride < (int64_t)la3d_mask_bits_words(H, W))))
    return refuse("la3d_mask_stats_bits", "bad argument (0 <= frame_width <= W, bits 4-byte aligned, bits_plane_stride >= la3d_mask_bits_words(H, W))");
  if ((long long)H * W > (1LL << 20)) return refuse("la3d_mask_stats_bits", "the bit image must fit LDS (H*W <= 1048576)", LA3D_ERR_UNSUPPORTED);
  if (B == 0) return LA3D_SUCCESS;
  const int nwords = (int)la3d_mask_bits_words(H, W);
  const int vec = ((reinterpret_cast<uintptr_t>(bits) & 15) == 0 && bits_plane_stride % 4 == 0) ? 1 : 0;
  allow_big_lds(reinterpret_cast<const void*>(mask_stats_bits_kernel));
  hipLaunchKernelGGL(mask_stats_bits_kernel, dim3(B), dim3(256), (((size_t)nwords * 4 + 15) & ~(size_t)15) + 16, static_cast<hipStream_t>(stream),
                     bits, (long long)bits_plane_stride, vec, H, W, frame_width > 0 ? frame_width : W, nwords, boundary, stats);
  return check_launch("mask_stats_bits_kernel");
}

int la3d_pack_rle_bits(const int32_t* counts, const int64_t* offsets, int B, int H, int W, int W_out, uint32_t* bits,
                       int64_t bits_plane_stride, int32_t* area, void* stream) {
  const BitsOut c = bits_out_uniform(H, W, W_out, bits, bits_plane_stride, area);
  const int rc = ann_check("la3d_pack_rle_bits", counts, offsets, offsets, B, W, c);
  if (rc != PACK_LAUNCH) return pack_done(rc);
  // (the block totals of the column scan, as in la3d_rle_decode: word-aligned rows only)
  const int ntx = W_out / 32;
  const int scan_words = (W_out % 32 == 0) ? ((NT_DEC / ntx > 2 ? NT_DEC / ntx : 2) * ntx) : 0;
  return pack_rle_launch<false>("la3d_pack_rle_bits", "pack_rle_bits_kernel", counts, offsets, B, scan_words, c, stream);
}

int la3d_pack_poly_bits(const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, int B, int H, int W, int W_out,
                        uint32_t* bits, int64_t bits_plane_stride, int32_t* area, void* stream) {
  const BitsOut c = bits_out_uniform(H, W, W_out, bits, bits_plane_stride, area);
  const int rc = ann_check("la3d_pack_poly_bits", poly_xy, ring_offsets, inst_rings, B, W, c);
  if (rc != PACK_LAUNCH) return pack_done(rc);
  return pack_poly_launch<false>("la3d_pack_poly_bits", "pack_poly_bits_kernel", poly_xy, ring_offsets, inst_rings, B, c, stream);
}

int la3d_pack_rle_bits_frames(const int32_t* counts, const int64_t* offsets, const la3d_frame* frames, int32_t P, int H, int W,
                              const int32_t* image_index, int B, uint32_t* bits, const int64_t* bits_offsets, int32_t* area,
                              void* stream) {
  const BitsOut c = bits_out_frames(frames, P, H, W, image_index, bits, bits_offsets, area);
  const int rc = ann_frames_check("la3d_pack_rle_bits_frames", counts, offsets, offsets, B, c);
  if (rc != PACK_LAUNCH) return pack_done(rc);
  // every frame of the call has at most (W + 31) / 32 words per row: room for two block rows of the widest, NT_DEC items otherwise
  const int ntx = (W + 31) / 32;
  const int scan_words = 2 * ntx > NT_DEC ? 2 * ntx : NT_DEC;
  return pack_rle_launch<true>("la3d_pack_rle_bits_frames", "pack_rle_bits_frames_kernel", counts, offsets, B, scan_words, c, stream);
}

int la3d_pack_poly_bits_frames(const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, const la3d_frame* frames,
                               int32_t P, int H, int W, const int32_t* image_index, int B, uint32_t* bits, const int64_t* bits_offsets,
                               int32_t* area, void* stream) {
  const BitsOut c = bits_out_frames(frames, P, H, W, image_index, bits, bits_offsets, area);
  const int rc = ann_frames_check("la3d_pack_poly_bits_frames", poly_xy, ring_offsets, inst_rings, B, c);
  if (rc != PACK_LAUNCH) return pack_done(rc);
  return pack_poly_launch<true>("la3d_pack_poly_bits_frames", "pack_poly_bits_frames_kernel", poly_xy, ring_offsets, inst_rings, B, c, stream);
}

int la3d_pack_crop_bits(const uint8_t* crops, int64_t crop_stride, int32_t row_pitch, int32_t pixel_step, int S, int threshold,
                        const int32_t* place, int B, int H, int W, int W_out, uint32_t* bits, int64_t bits_plane_stride, int32_t* area,
                        void* stream) {
  const char* who = "la3d_pack_crop_bits";
  CropSrc src;
  const int bad = crop_source(who, crops, crop_stride, row_pitch, pixel_step, S, threshold, place, B, &src);
  if (bad != LA3D_SUCCESS) return bad;
  const BitsOut c = bits_out_uniform(H, W, W_out, bits, bits_plane_stride, area);
  const int rc = ann_check(who, crops, place, place, B, W, c);
  if (rc != PACK_LAUNCH) return pack_done(rc);
  return pack_crop_launch<false>(src, B, c, stream);
}

int la3d_pack_crop_bits_frames(const uint8_t* crops, int64_t crop_stride, int32_t row_pitch, int32_t pixel_step, int S, int threshold,
                               const int32_t* place, const la3d_frame* frames, int32_t P, int H, int W, const int32_t* image_index, int B,
                               uint32_t* bits, const int64_t* bits_offsets, int32_t* area, void* stream) {
  const char* who = "la3d_pack_crop_bits_frames";
  CropSrc src;
  const int bad = crop_source(who, crops, crop_stride, row_pitch, pixel_step, S, threshold, place, B, &src);
  if (bad != LA3D_SUCCESS) return bad;
  const BitsOut c = bits_out_frames(frames, P, H, W, image_index, bits, bits_offsets, area);
  const int rc = ann_frames_check(who, crops, place, place, B, c);
  if (rc != PACK_LAUNCH) return pack_done(rc);
  return pack_crop_launch<true>(src, B, c, stream);
}

int la3d_pack_label_bits(const void* labels, int dtype, int64_t plane_stride, int P, int H, int W, int W_out,
                         const int32_t* inst_offsets, const int32_t* inst_label, int B, uint32_t* bits, int64_t bits_plane_stride,
                         int32_t* area, void* stream) {
  const char* who = "la3d_pack_label_bits";
  static const PackWords say = {"bad argument (B, P >= 0, H, W > 0, W_out >= W)",
                                "frame or batch too large (H*W_out <= 2^28, P * ceil(H*W_out / 8192) < 2^31)",
                                "NULL labels, inst_offsets, inst_label or bits", nullptr, "label plane stride smaller than H*W", BITS_STRIDE};
  if (dtype != LA3D_LABEL_U8 && dtype != LA3D_LABEL_U16 && dtype != LA3D_LABEL_I32 && dtype != LA3D_LABEL_RGB8) return refuse(who, LABEL_DTYPE);
  const long long plane = plane_items(H, W_out);
  const int rc = pack_check(who, say, B, P, W, B > 0 && P > 0, plane > (1LL << 28) || (long long)P * ((plane + 8191) / 8192) > 0x7fffffffLL, false,
                            {{bits, 3, BITS_4}, {labels, dtype == LA3D_LABEL_I32 ? 3u : dtype == LA3D_LABEL_U16 ? 1u : 0u, "labels not aligned to their element size"},
                             {inst_offsets, 3, LABEL_PTRS_4}, {inst_label, 3, LABEL_PTRS_4}, {area, 3, LABEL_PTRS_4, true}},
                            plane_stride, bits_out_uniform(H, W, W_out, bits, bits_plane_stride, area));
  if (rc != PACK_LAUNCH) return pack_done(rc);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cleared = clear_area(area, B, s);
  if (cleared != LA3D_SUCCESS) return cleared;
  return with_kind(dtype, [&](auto k) {
    return pack_labels_launch<decltype(k)::value>(labels, plane_stride, P, H, W, W_out, inst_offsets, inst_label, B, bits, bits_plane_stride, area, s);
  });
}

int la3d_pack_label_bits_frames(const void* labels, int dtype, const la3d_frame* frames, int32_t P, int H, int W,
                                const int32_t* inst_offsets, const int32_t* inst_label, int B, uint32_t* bits,
                                const int64_t* bits_offsets, int32_t* area, void* stream) {
  const char* who = "la3d_pack_label_bits_frames";
  static const char* const p8 = "frames or bits_offsets not an 8-byte aligned pointer";
  static const PackWords say = {SIZES_FRAMES, "bounds or batch too large (H * roundup32(W) <= 2^28, P * ceil(H * roundup32(W) / 8192) < 2^31)",
                                "NULL labels, frames, inst_offsets, inst_label, bits or bits_offsets", nullptr, nullptr, nullptr};
  if (dtype != LA3D_LABEL_U8 && dtype != LA3D_LABEL_U16 && dtype != LA3D_LABEL_I32 && dtype != LA3D_LABEL_RGB8) return refuse(who, LABEL_DTYPE);
  const BitsOut c = bits_out_frames(frames, P, H, W, nullptr, bits, bits_offsets, area);   // (the image of a row: inst_offsets)
  const long long words = bounds_words(H, W), chunks = (words + 255) / 256;
  const int rc = pack_check(who, say, B, P, W, B > 0 && P > 0, words > (1LL << 23) || (long long)P * chunks > 0x7fffffffLL, false,
                            {{labels, 15, "labels not a 16-byte aligned pointer"}, {bits, 3, BITS_4}, {frames, 7, p8}, {bits_offsets, 7, p8},
                             {inst_offsets, 3, LABEL_PTRS_4}, {inst_label, 3, LABEL_PTRS_4}, {area, 3, LABEL_PTRS_4, true}}, 0, c);
  if (rc != PACK_LAUNCH) return pack_done(rc);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cleared = clear_area(area, B, s);
  if (cleared != LA3D_SUCCESS) return cleared;
  return with_kind(dtype, [&](auto k) { return pack_labels_frames_launch<decltype(k)::value>(labels, (int)chunks, inst_offsets, inst_label, B, c, s); });
}

int la3d_pack_mask_bits_frames(const uint8_t* mask, const la3d_frame* frames, int32_t P, int H, int W, const int32_t* image_index,
                               const int64_t* src_offsets, const int32_t* src_pitch, int B, uint32_t* bits, const int64_t* bits_offsets,
                               int32_t* area, void* stream) {
  return pack_masks_frames("la3d_pack_mask_bits_frames", mask, PK_U8, 0.0f, frames, P, H, W, image_index, src_offsets, src_pitch, B, bits,
                           bits_offsets, area, stream);
}

int la3d_pack_logits_bits_frames(const void* logits, int dtype, float threshold, const la3d_frame* frames, int32_t P, int H, int W,
                                 const int32_t* image_index, const int64_t* src_offsets, const int32_t* src_pitch, int B, uint32_t* bits,
                                 const int64_t* bits_offsets, int32_t* area, void* stream) {
  if (dtype != LA3D_DTYPE_F32 && dtype != LA3D_DTYPE_F16 && dtype != LA3D_DTYPE_BF16)
    return refuse("la3d_pack_logits_bits_frames", "unknown dtype (LA3D_DTYPE_F32, LA3D_DTYPE_F16 or LA3D_DTYPE_BF16)");
  const int kind = dtype == LA3D_DTYPE_F32 ? PK_F32 : dtype == LA3D_DTYPE_F16 ? PK_F16 : PK_BF16;
  return pack_masks_frames("la3d_pack_logits_bits_frames", logits, kind, threshold, frames, P, H, W, image_index, src_offsets, src_pitch, B,
                           bits, bits_offsets, area, stream);
}

}  // extern "C"
