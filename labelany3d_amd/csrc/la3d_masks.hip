// la3d_masks.hip - whole-frame depth_to_points (src/util.py:52-75), row padding, and the mask side of the path: decode and the
// filter statistics of u8 planes, COCO run lengths and polygon parts (src/util.py:291-415) as kernels of their own (the fit engines decode
// inside the fit launch).  Split out of la3d_aux.hip in round 6.
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

using namespace la3d;

namespace {
// ------------------------------------------------------------------------------------------
// depth_to_points for a whole frame (write-bound: 4 B in, 24 B out per pixel)
// ------------------------------------------------------------------------------------------
struct UnprojParams {
  double Kinv[9];
  double R[9];
  double t[3];
  int has_rt;
  int H, W, HW;
  float rcpW;
};

// One wave turns 64 consecutive pixels into 64 points per step.  The points go through a per-wave LDS stage so that the wave
// writes its 1536 (f64) / 768 (f32) contiguous output bytes as whole 16-byte non-temporal stores (the output is written once and
// read by somebody else: measured 64 / 256 / 1024 frames of 640x480 -> f64: 148 / 541 / 1921 us with plain per-lane stores,
// 89 / 477 / 1656 us this way = 6.1 / 4.6 / 5.3 TB/s; a device copy of the same size moves 5.3 / 4.4 / 4.7 TB/s, a pure fill
// 6.4 / 6.8 / 6.8 TB/s: profiles/r03/r03_unproject.txt).  vec16: every frame's output base is
// 16-byte aligned.  kinv: the frame's inverse intrinsics in LDS.
template <typename OutT>
__device__ inline void unproject_frame(const float* __restrict__ dp, OutT* __restrict__ op, const double* kinv, OutT* sl,
                                       const UnprojParams& p, int first, int stride, int lane, bool vec16) {
  constexpr int N16 = 64 * 3 * (int)sizeof(OutT) / 16;   // 16-byte pieces per 64 points
  for (int i0 = first; i0 < p.HW; i0 += stride) {   // wave-uniform trip count
    const int i = i0 + lane;
    double w[3] = {0, 0, 0};
    if (i < p.HW) {
      unsigned u, v;
      pix_uv((unsigned)i, p.W, p.rcpW, &u, &v);
      // (plain load: a depth plane that a previous kernel left in the cache should be found there)
      const double d = (double)dp[i], ud = (double)u, vd = (double)v;
      // (D * Kinv) @ [u, v, 1]   - precedence as in the reference, src/util.py:71-72
      double q[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) q[r] = (d * kinv[r * 3]) * ud + (d * kinv[r * 3 + 1]) * vd + (d * kinv[r * 3 + 2]);
      if (p.has_rt) {   // R @ p + t  (:74)
#pragma unroll
        for (int r = 0; r < 3; ++r) w[r] = p.R[r * 3] * q[0] + p.R[r * 3 + 1] * q[1] + p.R[r * 3 + 2] * q[2] + p.t[r];
      } else {
        // R = I, t = 0 in the reference still multiplies: 1*x + 0*y + 0*z + 0 - a NaN / inf component poisons its
        // neighbours exactly as there
        w[0] = 1.0 * q[0] + 0.0 * q[1] + 0.0 * q[2] + 0.0;
        w[1] = 0.0 * q[0] + 1.0 * q[1] + 0.0 * q[2] + 0.0;
        w[2] = 0.0 * q[0] + 0.0 * q[1] + 1.0 * q[2] + 0.0;
      }
    }
    sl[lane * 3] = (OutT)w[0]; sl[lane * 3 + 1] = (OutT)w[1]; sl[lane * 3 + 2] = (OutT)w[2];
    // lanes exchange through LDS: the hardware completes a wave's LDS operations in order, but the compiler must be told that the
    // reads below depend on OTHER lanes' writes (it can prove that 3 lane + 1 never equals 64 + lane and would hoist that read)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const long long base = (long long)i0 * 3, lim = (long long)p.HW * 3;
    if (vec16 && i0 + 64 <= p.HW) {   // uniform
      const u32x4* s16 = reinterpret_cast<const u32x4*>(sl);
      u32x4* o16 = reinterpret_cast<u32x4*>(op + base);
#pragma unroll
      for (int k = 0; k < (N16 + 63) / 64; ++k)
        if (k * 64 + lane < N16) __builtin_nontemporal_store(s16[k * 64 + lane], o16 + k * 64 + lane);
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (base + k * 64 + lane < lim) __builtin_nontemporal_store(sl[k * 64 + lane], op + base + k * 64 + lane);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

template <typename OutT>
__global__ __launch_bounds__(256) void unproject_kernel(const float* __restrict__ depth, OutT* __restrict__ out,
                                                        const UnprojParams p, int vec16) {
  __shared__ double kinv[9];
  __shared__ __attribute__((aligned(16))) OutT stage[4][192];
  if (threadIdx.x < 9) kinv[threadIdx.x] = p.Kinv[threadIdx.x];   // (inverted on the host: la3d_unproject)
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unproject_frame<OutT>(depth, out, kinv, stage[wave], p, blockIdx.x * blockDim.x + wave * 64, gridDim.x * blockDim.x, lane, vec16 != 0);
}

// P frames in one launch: blockIdx.y = frame; the frame's K is inverted by one thread (device inv3 = the host routine's elimination)
template <typename OutT>
__global__ __launch_bounds__(256) void unproject_batch_kernel(const float* __restrict__ depth, const double* __restrict__ K,
                                                              int k_stride, OutT* __restrict__ out, const UnprojParams p, int vec16) {
  __shared__ double kinv[9];
  __shared__ __attribute__((aligned(16))) OutT stage[4][192];
  if (threadIdx.x == 0) inv3(K + (long long)blockIdx.y * k_stride, kinv);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unproject_frame<OutT>(depth + (long long)blockIdx.y * p.HW, out + (long long)blockIdx.y * p.HW * 3, kinv, stage[wave], p,
                        blockIdx.x * blockDim.x + wave * 64, gridDim.x * blockDim.x, lane, vec16 != 0);
}

// Depth rows padded on the right with zeros: [rows][W] f32 -> [rows][Wp] f32, Wp % 4 == 0 (la3d_fit_args::frame_width: frames whose
// width is not a multiple of 32).  One 16-byte store per thread and step; the loads are 4-byte (a row of odd width starts anywhere),
// consecutive lanes read consecutive floats.
__global__ __launch_bounds__(256) void pad_rows_kernel(const float* __restrict__ src, long long rows, int W, int Wp, float* __restrict__ dst) {
  const int qpr = Wp >> 2;                                   // 16-byte groups per padded row
  const long long total = rows * qpr;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
    const long long r = g / qpr;
    const int c = (int)(g - r * qpr) * 4;
    const float* s = src + r * W + c;
    u32x4 v;   // (bit patterns: the store is a plain 16-byte move)
    v.x = c < W ? __float_as_uint(s[0]) : 0u; v.y = c + 1 < W ? __float_as_uint(s[1]) : 0u;
    v.z = c + 2 < W ? __float_as_uint(s[2]) : 0u; v.w = c + 3 < W ? __float_as_uint(s[3]) : 0u;
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(dst) + g);
  }
}

__global__ __launch_bounds__(256) void mask_counts_kernel(const unsigned char* __restrict__ mask, int HW, int vec,
                                                          int* __restrict__ counts) {
  __shared__ int part[4];
  const unsigned char* m = mask + (long long)blockIdx.x * HW;
  int n = 0;
  if (vec) {
    const uint4* m4 = reinterpret_cast<const uint4*>(m);
    for (int g = threadIdx.x; g < HW / 16; g += 256) {
      const uint4 w = m4[g];
      n += __popc(nz4(w.x)) + __popc(nz4(w.y)) + __popc(nz4(w.z)) + __popc(nz4(w.w));
    }
  } else {
    for (int i = threadIdx.x; i < HW; i += 256) n += m[i] ? 1 : 0;
  }
  n = wave_sum_i(n);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

constexpr int NT_DEC = 512;   // decode kernels: 8 waves per workgroup (four workgroups per CU by LDS: 32 waves keep the stores coming)

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
struct BitsOut {              // where the planes of a call go (kernel argument)
  unsigned* bits;
  long long stride;           // uniform form: words between planes
  const long long* offsets;   // frames form: words from bits to the plane of each instance
  int* area;                  // [B] or NULL
  const la3d_frame* frames;   // frames form: the table, P rows
  const int* image_index;
  int P;
  int H, W;                   // uniform form: the frame as stored (W = W_out); frames form: the bounds
  int frame_w;                // uniform form: the image columns where the rows are padded (0: none)
  int lds_words;              // words of the bit image the launch reserved (uniform form: the plane's)
  int vec;                    // uniform form: every plane 16-byte aligned
};
struct PlaneGeo { int H, W, fw, nwords, vec; unsigned* out; };

// The geometry and the plane of instance b.  Frames form: every value that decides an address comes through a scalar load and is
// checked BEFORE an address is formed from it - the image index, then the frame row (frame_row_ok: the check the fit makes), then
// the plane's offset (>= 0, a multiple of 4: the rule of the fit).  false: the instance is refused - nothing is written for it.
template <bool FRAMES>
__device__ inline bool plane_geometry(const BitsOut& c, int b, PlaneGeo* g) {
  if constexpr (FRAMES) {
    const int img = __builtin_amdgcn_readfirstlane(c.image_index[b]);
    if ((unsigned)img >= (unsigned)c.P) return false;
    const FrameRow r = frame_row_load(c.frames + img);
    if (!frame_row_ok(r, c.H, c.W)) return false;
    const long long oo = poly_uniform(c.offsets[b]);
    if (oo < 0 || (oo & 3) != 0) return false;
    g->H = r.H; g->W = r.W; g->fw = r.fw;
    g->nwords = (r.H * r.W) >> 5;   // (<= lds_words: H <= bound, W <= bound, W % 32 == 0)
    g->vec = 1;                     // (bits is 16-byte aligned - checked on the host - and the offset a multiple of 4)
    g->out = c.bits + oo;
  } else {
    g->H = c.H; g->W = c.W; g->fw = c.frame_w; g->nwords = c.lds_words; g->vec = c.vec;
    g->out = c.bits + (long long)b * c.stride;
  }
  return true;
}

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

// The reference's filter quantities (mask_stats) for polygon annotations without materialising a plane: rasterise into
// LDS, count there.  Dynamic LDS: bit image, side stage, flags (64 B), per-row counts (H ints), 20 ints.
__global__ __launch_bounds__(256) void mask_stats_poly_kernel(const int* __restrict__ xy, const long long* __restrict__ ring_off,
                                                              const long long* __restrict__ inst_rings, int H, int W, int nwords,
                                                              int boundary, int* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  const size_t bit_bytes = ((size_t)nwords * 4 + 15) & ~(size_t)15;
  PolySide* stage = reinterpret_cast<PolySide*>(smem + bit_bytes);
  unsigned* flags = reinterpret_cast<unsigned*>(smem + bit_bytes + POLY_STAGE_BYTES);
  int* rowcnt = reinterpret_cast<int*>(smem + bit_bytes + POLY_STAGE_BYTES + 64);
  int* red = rowcnt + H;
  const int tid = threadIdx.x;
  (void)poly_to_bits<256>(xy, ring_off, inst_rings[blockIdx.x], inst_rings[blockIdx.x + 1], stage, flags, bits, nwords, H, W, tid);
  int o4[4];
  bits_stats_256(bits, H, W, boundary, rowcnt, red, tid, o4);
  if (tid == 0) {
    int* o = stats + (long long)blockIdx.x * 4;
    o[0] = o4[0]; o[1] = o4[1]; o[2] = o4[2]; o[3] = o4[3];
  }
}

// The quantities of the reference's instance filter (src/util.py:291-335, :367-376) per mask plane:
// stats[0] = area, [1] = rows holding a pixel, [2] = last row - first row + 1, [3] = pixels inside the four
// boundary strips of `boundary` px (corners counted twice, as analyze_mask does).
__global__ __launch_bounds__(256) void mask_stats_kernel(const unsigned char* __restrict__ mask, int H, int W, int boundary,
                                                         int* __restrict__ stats) {
  __shared__ int red[4][4];
  const unsigned char* m = mask + (long long)blockIdx.x * H * W;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int area = 0, rows = 0, first = H, last = -1, trunc = 0;
  for (int r = wave; r < H; r += 4) {  // one wave per row
    int cnt = 0, edge = 0;
    for (int c = lane; c < W; c += 64) {
      const int on = m[(long long)r * W + c] ? 1 : 0;
      cnt += on;
      if (on) edge += (c < boundary ? 1 : 0) + (c >= W - boundary ? 1 : 0);
    }
    cnt = wave_sum_i(cnt);
    edge = wave_sum_i(edge);
    area += cnt;
    trunc += edge;
    if (r < boundary || r >= H - boundary) trunc += (r < boundary && r >= H - boundary) ? 2 * cnt : cnt;
    if (cnt) { rows += 1; first = min(first, r); last = max(last, r); }
  }
  if (lane == 0) { red[wave][0] = area; red[wave][1] = rows; red[wave][2] = first; red[wave][3] = last; }
  __shared__ int tr[4];
  if (lane == 0) tr[wave] = trunc;
  __syncthreads();
  if (tid == 0) {
    int a = 0, rw = 0, f = H, l = -1, t = 0;
    for (int w = 0; w < 4; ++w) { a += red[w][0]; rw += red[w][1]; f = min(f, red[w][2]); l = max(l, red[w][3]); t += tr[w]; }
    int* o = stats + (long long)blockIdx.x * 4;
    o[0] = a; o[1] = rw; o[2] = (l >= f) ? l - f + 1 : 0; o[3] = t;
  }
}

// ---- the same four quantities, wide loads and run-length input -------------------------------------------------
// Shared tail: rowv[r] != 0 <=> row r holds a pixel.  Returns rows / first / last over the workgroup (256 threads);
// red: LDS, 3 x 4 ints.
__device__ inline void rows_summary(const int* rowv, int H, int* red, int tid, int* rows_out, int* span_out) {
  const int lane = tid & 63, wave = tid >> 6;
  int rows = 0, first = H, last = -1;
  for (int r = tid; r < H; r += 256)
    if (rowv[r] != 0) { rows += 1; first = min(first, r); last = max(last, r); }
  rows = wave_sum_i(rows);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { first = min(first, __shfl_xor(first, o)); last = max(last, __shfl_xor(last, o)); }
  if (lane == 0) { red[wave] = rows; red[4 + wave] = first; red[8 + wave] = last; }
  __syncthreads();
  int rw = 0, f = H, l = -1;
  for (int w = 0; w < 4; ++w) { rw += red[w]; f = min(f, red[4 + w]); l = max(l, red[8 + w]); }
  *rows_out = rw;
  *span_out = (l >= f) ? l - f + 1 : 0;
}

// u8 planes with W % 16 == 0 and 16-byte aligned planes: 16 pixels per load, four loads in flight per lane, per-row
// pixel counts accumulated in LDS (one atomic per non-empty group).  Dynamic LDS: H ints.
__global__ __launch_bounds__(256) void mask_stats_vec_kernel(const unsigned char* __restrict__ mask, int H, int W, int boundary,
                                                             int* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* rowcnt = reinterpret_cast<int*>(smem);
  __shared__ int red[12];
  __shared__ int tot[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int r = tid; r < H; r += 256) rowcnt[r] = 0;
  __syncthreads();
  const u32x4* m4 = reinterpret_cast<const u32x4*>(mask + (long long)blockIdx.x * H * W);
  const int gpr = W >> 4, ngroups = H * gpr;
  const int step_row = 256 / gpr, step_col = 256 % gpr;
  const int bc = min(boundary, W);
  int row = tid / gpr, col = tid - row * gpr;
  int area = 0, edge = 0;
#pragma unroll 4
  for (int g = tid; g < ngroups; g += 256) {
    const u32x4 w = __builtin_nontemporal_load(m4 + g);
    const unsigned pat = nz4(w.x) | (nz4(w.y) << 4) | (nz4(w.z) << 8) | (nz4(w.w) << 12);
    if (pat) {
      const int c0 = col << 4, n = __popc(pat);
      area += n;
      atomicAdd(&rowcnt[row], n);
      const int nlo = min(max(bc - c0, 0), 16), fhi = min(max(W - bc - c0, 0), 16);
      edge += __popc(pat & ((1u << nlo) - 1u)) + __popc(pat & (0xffffu & ~((1u << fhi) - 1u)));
    }
    col += step_col; row += step_row;
    if (col >= gpr) { col -= gpr; ++row; }
  }
  __syncthreads();
  // top / bottom strips from the row counts (a row inside both strips counts twice, as m[:b].sum() + m[-b:].sum() does)
  const int br = min(boundary, H);
  for (int r = tid; r < H; r += 256) {
    const int k = (r < br ? 1 : 0) + (r >= H - br ? 1 : 0);
    if (k) edge += k * rowcnt[r];
  }
  area = wave_sum_i(area);
  edge = wave_sum_i(edge);
  if (lane == 0) { tot[wave][0] = area; tot[wave][1] = edge; }
  int rows, span;
  rows_summary(rowcnt, H, red, tid, &rows, &span);  // has the barrier that publishes tot
  if (tid == 0) {
    int* o = stats + (long long)blockIdx.x * 4;
    o[0] = tot[0][0] + tot[1][0] + tot[2][0] + tot[3][0];
    o[1] = rows; o[2] = span;
    o[3] = tot[0][1] + tot[1][1] + tot[2][1] + tot[3][1];
  }
}

// COCO run lengths (column-major, zeros first): no plane is decoded.  A ones-run is the interval [s, e) of the
// column-major pixel index i = col * H + row, so every quantity is interval arithmetic: area = sum of lengths; the
// left / right strips are the index ranges [0, b*H) and [(W-b)*H, W*H); the top / bottom strips are the residues
// i mod H in [0, b) and [H-b, H), counted in closed form; row presence goes through a difference array over rows
// (two LDS atomics per run) and one prefix scan.  Dynamic LDS: H + 1 ints.
__device__ inline long long strip_rows_below(long long x, int H, int br) {  // pixels i < x with i mod H in the two row strips
  const long long q = x / H;
  const int r = (int)(x - q * H);
  return q * 2 * br + min(r, br) + max(0, r - (H - br));
}

__global__ __launch_bounds__(256) void mask_stats_rle_kernel(const int* __restrict__ counts, const long long* __restrict__ offsets,
                                                             int H, int W, int boundary, int* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* diff = reinterpret_cast<int*>(smem);  // [H + 1]
  __shared__ int red[12];
  __shared__ unsigned wtot[4];
  __shared__ long long tot[4][2];
  __shared__ int full;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long o0 = offsets[blockIdx.x];
  const int nr = (int)(offsets[blockIdx.x + 1] - o0);
  const int* cnt = counts + o0;
  const long long HW = (long long)H * W;
  for (int r = tid; r <= H; r += 256) diff[r] = 0;
  if (tid == 0) full = 0;
  const int bc = min(boundary, W), br = min(boundary, H);
  const long long left_end = (long long)bc * H, right_beg = (long long)(W - bc) * H;
  long long area = 0, edge = 0;
  unsigned long long carry = 0;
  for (int c0 = 0; c0 < nr; c0 += 256) {
    const int j = c0 + tid;
    unsigned len = 0;
    if (j < nr) { const int v = cnt[j]; len = v > 0 ? (unsigned)v : 0u; }
    unsigned incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    __syncthreads();  // previous step's readers of wtot are done; the zeroing of diff is ordered
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    unsigned long long base = carry, total = 0;
    for (int w = 0; w < 4; ++w) { if (w < wave) base += wtot[w]; total += wtot[w]; }
    const long long s = (long long)(base + incl - len);
    carry += total;
    if ((j & 1) && len > 0 && s < HW) {
      const long long e = min(s + (long long)len, HW);
      area += e - s;
      edge += max(0LL, min(e, left_end) - s) + max(0LL, e - max(s, right_beg));
      edge += strip_rows_below(e, H, br) - strip_rows_below(s, H, br);
      if (e - s >= H) {
        full = 1;  // every row holds a pixel
      } else {
        const int r0 = (int)(s % H), r1 = (int)((e - 1) % H);
        if (r0 <= r1) { atomicAdd(&diff[r0], 1); atomicAdd(&diff[r1 + 1], -1); }
        else { atomicAdd(&diff[r0], 1); atomicAdd(&diff[H], -1); atomicAdd(&diff[0], 1); atomicAdd(&diff[r1 + 1], -1); }
      }
    }
    if (carry >= (unsigned long long)HW) break;  // uniform: later runs fall outside the frame
  }
  __syncthreads();
  // prefix scan of the difference array in place (chunk per thread, chunk sums scanned through LDS)
  const int per = (H + 255) / 256, rb = min(tid * per, H), re = min(rb + per, H);
  int csum = 0;
  for (int r = rb; r < re; ++r) csum += diff[r];
  int incl = csum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wtot[wave] = (unsigned)incl;
  __syncthreads();
  int run = incl - csum;
  for (int w = 0; w < wave; ++w) run += (int)wtot[w];
  const int all_rows = full;
  for (int r = rb; r < re; ++r) { run += diff[r]; diff[r] = (run > 0 || all_rows) ? 1 : 0; }
  // publish the sums, then rows / span (rows_summary's barrier orders the diff writes and tot)
  for (int o = 32; o > 0; o >>= 1) { area += __shfl_xor(area, o); edge += __shfl_xor(edge, o); }
  if (lane == 0) { tot[wave][0] = area; tot[wave][1] = edge; }
  __syncthreads();
  int rows, span;
  rows_summary(diff, H, red, tid, &rows, &span);
  if (tid == 0) {
    int* o = stats + (long long)blockIdx.x * 4;
    o[0] = (int)(tot[0][0] + tot[1][0] + tot[2][0] + tot[3][0]);
    o[1] = rows; o[2] = span;
    o[3] = (int)(tot[0][1] + tot[1][1] + tot[2][1] + tot[3][1]);
  }
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

// host-side 3x3 inverse (same elimination as the device-side inv3)
void inv3_host(const double* A, double* X) {
  double a[3][6];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { a[i][j] = A[i * 3 + j]; a[i][3 + j] = (i == j) ? 1.0 : 0.0; }
  for (int c = 0; c < 3; ++c) {
    int piv = c;
    for (int r = c + 1; r < 3; ++r) if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
    if (piv != c) for (int j = 0; j < 6; ++j) { double t = a[c][j]; a[c][j] = a[piv][j]; a[piv][j] = t; }
    const double inv = 1.0 / a[c][c];
    for (int r = c + 1; r < 3; ++r) { const double f = a[r][c] * inv; for (int j = c; j < 6; ++j) a[r][j] -= f * a[c][j]; }
  }
  for (int j = 0; j < 3; ++j)
    for (int r = 2; r >= 0; --r) {
      double s = a[r][3 + j];
      for (int k = r + 1; k < 3; ++k) s -= a[r][k] * X[k * 3 + j];
      X[r * 3 + j] = s / a[r][r];
    }
}

}  // namespace

// ==========================================================================================
// C-ABI
// ==========================================================================================
extern "C" {

int la3d_unproject(const float* depth, const double* K9, const double* Rt12, int H, int W, void* out,
                   int out_is_f64, void* stream) {
  if (!depth || !K9 || !out || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL / 4) {
    set_err("la3d_unproject: bad argument");
    return LA3D_ERR_ARG;
  }
  UnprojParams p;
  inv3_host(K9, p.Kinv);
  p.has_rt = Rt12 != nullptr;
  for (int i = 0; i < 9; ++i) p.R[i] = Rt12 ? Rt12[i] : ((i % 4 == 0) ? 1.0 : 0.0);
  for (int i = 0; i < 3; ++i) p.t[i] = Rt12 ? Rt12[9 + i] : 0.0;
  p.H = H; p.W = W; p.HW = H * W; p.rcpW = 1.0f / (float)W;
  const int blocks = (p.HW + 255) / 256 < 2048 ? (p.HW + 255) / 256 : 2048;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int vec16 = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (out_is_f64) hipLaunchKernelGGL(unproject_kernel<double>, dim3(blocks), dim3(256), 0, s, depth, static_cast<double*>(out), p, vec16);
  else hipLaunchKernelGGL(unproject_kernel<float>, dim3(blocks), dim3(256), 0, s, depth, static_cast<float*>(out), p, vec16);
  return check_launch("unproject_kernel");
}

int la3d_unproject_batch(const float* depth, const double* K, int32_t k_stride, const double* Rt12, int P, int H, int W, void* out,
                         int out_is_f64, void* stream) {
  if (!depth || !K || !out || P < 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL / 4 || (k_stride != 0 && k_stride < 9) ||
      P > 65535) {
    set_err("la3d_unproject_batch: bad argument (P <= 65535)");
    return LA3D_ERR_ARG;
  }
  if (P == 0) return LA3D_SUCCESS;
  UnprojParams p;
  for (int i = 0; i < 9; ++i) p.Kinv[i] = 0.0;
  p.has_rt = Rt12 != nullptr;
  for (int i = 0; i < 9; ++i) p.R[i] = Rt12 ? Rt12[i] : ((i % 4 == 0) ? 1.0 : 0.0);
  for (int i = 0; i < 3; ++i) p.t[i] = Rt12 ? Rt12[9 + i] : 0.0;
  p.H = H; p.W = W; p.HW = H * W; p.rcpW = 1.0f / (float)W;
  int bx = (p.HW + 255) / 256;
  // enough workgroups over all frames to fill the chip several times - but never fewer than 256 per frame: the ~2000 resident
  // workgroups then write into ~8 frames at a time instead of 64 (profiles/r05/r05_unproject_sweep.txt: 256 / 1024 frames of 640x480,
  // f64 out: 4.66 / 5.24 TB/s with 32 workgroups per frame, 5.41 / 5.78 with 256)
  int want = (8192 + P - 1) / P;
  if (want < 256) want = 256;
  if (bx > want) bx = want;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // 16-byte stores need every frame's output base 16-aligned: HW * 3 * sizeof(OutT) a multiple of 16
  const int vec16 = (reinterpret_cast<uintptr_t>(out) & 15) == 0 && ((long long)p.HW * 3 * (out_is_f64 ? 8 : 4)) % 16 == 0;
  if (out_is_f64) hipLaunchKernelGGL(unproject_batch_kernel<double>, dim3(bx, P), dim3(256), 0, s, depth, K, k_stride, static_cast<double*>(out), p, vec16);
  else hipLaunchKernelGGL(unproject_batch_kernel<float>, dim3(bx, P), dim3(256), 0, s, depth, K, k_stride, static_cast<float*>(out), p, vec16);
  return check_launch("unproject_batch_kernel");
}

int la3d_pad_rows(const float* src, int64_t rows, int W, int Wp, float* dst, void* stream) {
  if (rows < 0 || W <= 0 || Wp < W || Wp % 4 != 0 || (rows > 0 && (!src || !dst)) || (reinterpret_cast<uintptr_t>(dst) & 15)) {
    set_err("la3d_pad_rows: bad argument (Wp >= W, Wp % 4 == 0, dst 16-byte aligned)");
    return LA3D_ERR_ARG;
  }
  if (rows == 0) return LA3D_SUCCESS;
  const long long total = (long long)rows * (Wp / 4);
  const long long want = (total + 255) / 256;
  const int blocks = (int)(want < 8192 ? want : 8192);
  hipLaunchKernelGGL(pad_rows_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), src, (long long)rows, W, Wp, dst);
  return check_launch("pad_rows_kernel");
}

int la3d_mask_counts(const uint8_t* mask, int B, int H, int W, int32_t* counts, void* stream) {
  if (!mask || !counts || B < 0 || H <= 0 || W <= 0) {
    set_err("la3d_mask_counts: bad argument");
    return LA3D_ERR_ARG;
  }
  if (B == 0) return LA3D_SUCCESS;
  const int HW = H * W;
  const int vec = (HW % 16 == 0) && ((reinterpret_cast<uintptr_t>(mask) & 15) == 0);
  hipLaunchKernelGGL(mask_counts_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), mask, HW, vec, counts);
  return check_launch("mask_counts_kernel");
}

int la3d_rle_from_string_host(const char* s, int64_t len, int32_t* counts, int cap) {
  // pycocotools rleFrString (maskApi.c): 5-bit groups, char - 48, bit 5 = continuation, bit 4 of the last
  // group = sign; counts beyond the third are stored as a difference to the count two places earlier
  if (!s || len < 0 || (!counts && cap > 0)) return -1;
  int m = 0;
  int64_t pz = 0;
  while (pz < len && s[pz]) {
    long x = 0;
    int k = 0, more = 1;
    while (more) {
      if (pz >= len) return -1;
      const int c = s[pz] - 48;
      x |= (long)(c & 0x1f) << (5 * k);
      more = c & 0x20;
      ++pz; ++k;
      if (!more && (c & 0x10)) x |= -1L << (5 * k);
    }
    if (m > 2) x += counts[m - 2];
    if (m >= cap) return -1;
    counts[m++] = (int32_t)x;
  }
  return m;
}

int la3d_rle_decode(const int32_t* counts, const int64_t* offsets, int B, int H, int W, uint8_t* mask_out, void* stream) {
  if ((!counts && B > 0) || !offsets || !mask_out || B < 0 || H <= 0 || W <= 0 || (long long)H * W > (1LL << 20)) {
    set_err("la3d_rle_decode: bad argument (H*W <= 1048576)");
    return LA3D_ERR_ARG;
  }
  if (B == 0) return LA3D_SUCCESS;
  const int nwords = (H * W + 31) / 32;
  // behind the bit image: 16 words of wave totals, then the block totals of the column scan (word-aligned rows)
  const int scan_words = (W % 32 == 0) ? ((NT_DEC / (W / 32) > 2 ? NT_DEC / (W / 32) : 2) * (W / 32)) : 0;
  const size_t lds = (size_t)nwords * 4 + 64 + (size_t)scan_words * 4;
  if (lds > 160 * 1024 - 256) {
    set_err("la3d_rle_decode: frame too large for LDS");
    return LA3D_ERR_UNSUPPORTED;
  }
  allow_big_lds(reinterpret_cast<const void*>(rle_decode_kernel));
  hipLaunchKernelGGL(rle_decode_kernel, dim3(B), dim3(NT_DEC), lds, static_cast<hipStream_t>(stream), counts,
                     reinterpret_cast<const long long*>(offsets), H, W, nwords, scan_words, mask_out);
  return check_launch("rle_decode_kernel");
}

int la3d_poly_decode(const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, int B, int H, int W,
                     uint8_t* mask_out, void* stream) {
  if (((!poly_xy || !ring_offsets || !inst_rings || !mask_out) && B > 0) || B < 0 || H <= 0 || W <= 0 ||
      (long long)H * W > (1LL << 20)) {
    set_err("la3d_poly_decode: bad argument (H*W <= 1048576)");
    return LA3D_ERR_ARG;
  }
  if (B == 0) return LA3D_SUCCESS;
  const int nwords = (H * W + 31) / 32;
  const size_t lds = (((size_t)nwords * 4 + 15) & ~(size_t)15) + POLY_STAGE_BYTES + 64;
  allow_big_lds(reinterpret_cast<const void*>(poly_decode_kernel));
  hipLaunchKernelGGL(poly_decode_kernel, dim3(B), dim3(NT_DEC), lds, static_cast<hipStream_t>(stream), poly_xy,
                     reinterpret_cast<const long long*>(ring_offsets), reinterpret_cast<const long long*>(inst_rings), H, W, nwords,
                     mask_out);
  return check_launch("poly_decode_kernel");
}

int la3d_mask_stats_poly(const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, int B, int H, int W,
                         int boundary, int32_t* stats, void* stream) {
  if (((!poly_xy || !ring_offsets || !inst_rings || !stats) && B > 0) || B < 0 || H <= 0 || W <= 0 || boundary < 0 ||
      (long long)H * W > (1LL << 20)) {
    set_err("la3d_mask_stats_poly: bad argument (H*W <= 1048576)");
    return LA3D_ERR_ARG;
  }
  if (B == 0) return LA3D_SUCCESS;
  const int nwords = (H * W + 31) / 32;
  const size_t lds = (((size_t)nwords * 4 + 15) & ~(size_t)15) + POLY_STAGE_BYTES + 64 + (size_t)H * 4 + 128;
  if (lds > 160 * 1024 - 256) {
    set_err("la3d_mask_stats_poly: frame too large for LDS");
    return LA3D_ERR_UNSUPPORTED;
  }
  allow_big_lds(reinterpret_cast<const void*>(mask_stats_poly_kernel));
  hipLaunchKernelGGL(mask_stats_poly_kernel, dim3(B), dim3(256), lds, static_cast<hipStream_t>(stream), poly_xy,
                     reinterpret_cast<const long long*>(ring_offsets), reinterpret_cast<const long long*>(inst_rings), H, W, nwords,
                     boundary, stats);
  return check_launch("mask_stats_poly_kernel");
}

static void stats_lds_attr() {  // rows beyond 16 K need more than the default 64 KiB of dynamic LDS
  for (const void* k : {reinterpret_cast<const void*>(mask_stats_rle_kernel), reinterpret_cast<const void*>(mask_stats_vec_kernel)})
    allow_big_lds(k, 160 * 1024 - 1024);
}

int la3d_mask_stats(const uint8_t* mask, int B, int H, int W, int boundary, int32_t* stats, void* stream) {
  if (!mask || !stats || B < 0 || H <= 0 || W <= 0 || boundary < 0) {
    set_err("la3d_mask_stats: bad argument");
    return LA3D_ERR_ARG;
  }
  if (B == 0) return LA3D_SUCCESS;
  if (W % 16 == 0 && (reinterpret_cast<uintptr_t>(mask) & 15) == 0 && H <= 32768) {
    stats_lds_attr();
    hipLaunchKernelGGL(mask_stats_vec_kernel, dim3(B), dim3(256), (size_t)H * 4, static_cast<hipStream_t>(stream), mask, H, W,
                       boundary, stats);
    return check_launch("mask_stats_vec_kernel");
  }
  hipLaunchKernelGGL(mask_stats_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), mask, H, W, boundary, stats);
  return check_launch("mask_stats_kernel");
}

int la3d_mask_stats_rle(const int32_t* counts, const int64_t* offsets, int B, int H, int W, int boundary, int32_t* stats,
                        void* stream) {
  if ((!counts && B > 0) || !offsets || !stats || B < 0 || H <= 0 || W <= 0 || boundary < 0 || H > 32768 ||
      (long long)H * W > (1LL << 30)) {
    set_err("la3d_mask_stats_rle: bad argument (H <= 32768, H*W <= 2^30)");
    return LA3D_ERR_ARG;
  }
  if (B == 0) return LA3D_SUCCESS;
  stats_lds_attr();
  hipLaunchKernelGGL(mask_stats_rle_kernel, dim3(B), dim3(256), (size_t)(H + 1) * 4, static_cast<hipStream_t>(stream), counts,
                     reinterpret_cast<const long long*>(offsets), H, W, boundary, stats);
  return check_launch("mask_stats_rle_kernel");
}

}  // extern "C"

// ---- masks as bit planes ------------------------------------------------------------------
namespace {
// workgroups per plane: enough to cover `items` once, at most 64 (grid-stride inside the plane beyond that)
inline int plane_chunks(long long items) {
  const long long c = (items + 255) / 256;
  return (int)(c < 1 ? 1 : (c > 64 ? 64 : c));
}

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

// the argument checks the two packers share; 1 = nothing to do (B == 0)
int pack_bits_check(const void* src, long long plane_stride, int B, int H, int W, int W_out, const uint32_t* bits,
                    long long bits_plane_stride, const char* who) {
  char msg[200];
  const char* bad = nullptr;
  if (B < 0 || H <= 0 || W <= 0 || W_out < W) bad = "bad argument (B >= 0, H, W > 0, W_out >= W)";
  else if ((long long)H * W_out > (1LL << 28) || (long long)B * 64 > 0x7fffffffLL) bad = "frame or batch too large (H*W_out <= 2^28, B <= 2^25)";
  else if (B > 0 && (!src || !bits || (reinterpret_cast<uintptr_t>(bits) & 3))) bad = "NULL input or bits not a 4-byte aligned pointer";
  else if (B > 0 && plane_stride < (long long)H * W) bad = "input plane stride smaller than H*W";
  else if (B > 0 && bits_plane_stride < (long long)la3d_mask_bits_words(H, W_out)) bad = "bits_plane_stride is smaller than la3d_mask_bits_words(H, W_out)";
  if (bad) {
    snprintf(msg, sizeof(msg), "%s: %s", who, bad);
    set_err(msg);
    return LA3D_ERR_ARG;
  }
  return B == 0 ? 1 : LA3D_SUCCESS;
}
}  // namespace

extern "C" {

int la3d_pack_mask_bits(const uint8_t* mask, int64_t mask_plane_stride, int B, int H, int W, int W_out, uint32_t* bits,
                        int64_t bits_plane_stride, void* stream) {
  const int rc = pack_bits_check(mask, mask_plane_stride, B, H, W, W_out, bits, bits_plane_stride, "la3d_pack_mask_bits");
  if (rc != LA3D_SUCCESS) return rc < 0 ? rc : LA3D_SUCCESS;
  return pack_bits_launch<PK_U8>(mask, mask_plane_stride, 0.0f, B, H, W, W_out, bits, bits_plane_stride, static_cast<hipStream_t>(stream),
                                 "pack_mask_bits_kernel");
}

int la3d_pack_logits_bits(const void* logits, int dtype, int64_t plane_stride, float threshold, int B, int H, int W, int W_out,
                          uint32_t* bits, int64_t bits_plane_stride, void* stream) {
  if (dtype != LA3D_DTYPE_F32 && dtype != LA3D_DTYPE_F16 && dtype != LA3D_DTYPE_BF16) {
    set_err("la3d_pack_logits_bits: unknown dtype (LA3D_DTYPE_F32, LA3D_DTYPE_F16 or LA3D_DTYPE_BF16)");
    return LA3D_ERR_ARG;
  }
  if (B > 0 && logits && (reinterpret_cast<uintptr_t>(logits) & (dtype == LA3D_DTYPE_F32 ? 3 : 1))) {
    set_err("la3d_pack_logits_bits: logits not aligned to their element size");
    return LA3D_ERR_ARG;
  }
  const int rc = pack_bits_check(logits, plane_stride, B, H, W, W_out, bits, bits_plane_stride, "la3d_pack_logits_bits");
  if (rc != LA3D_SUCCESS) return rc < 0 ? rc : LA3D_SUCCESS;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == LA3D_DTYPE_F32) return pack_bits_launch<PK_F32>(logits, plane_stride, threshold, B, H, W, W_out, bits, bits_plane_stride, s, "pack_logits_bits_kernel");
  if (dtype == LA3D_DTYPE_F16) return pack_bits_launch<PK_F16>(logits, plane_stride, threshold, B, H, W, W_out, bits, bits_plane_stride, s, "pack_logits_bits_kernel");
  return pack_bits_launch<PK_BF16>(logits, plane_stride, threshold, B, H, W, W_out, bits, bits_plane_stride, s, "pack_logits_bits_kernel");
}

int la3d_unpack_mask_bits(const uint32_t* bits, int64_t bits_plane_stride, int B, int H, int W_in, int W, uint8_t* mask, void* stream) {
  if (B < 0 || H <= 0 || W <= 0 || W_in < W || (long long)H * W_in > (1LL << 28) || (long long)B * 64 > 0x7fffffffLL ||
      (B > 0 && (!bits || !mask || (reinterpret_cast<uintptr_t>(bits) & 3) || bits_plane_stride < (int64_t)la3d_mask_bits_words(H, W_in)))) {
    set_err("la3d_unpack_mask_bits: bad argument (W <= W_in, bits 4-byte aligned, bits_plane_stride >= la3d_mask_bits_words(H, W_in))");
    return LA3D_ERR_ARG;
  }
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
      (B > 0 && (!bits || !stats || (reinterpret_cast<uintptr_t>(bits) & 3) || bits_plane_stride < (int64_t)la3d_mask_bits_words(H, W)))) {
    set_err("la3d_mask_stats_bits: bad argument (0 <= frame_width <= W, bits 4-byte aligned, bits_plane_stride >= la3d_mask_bits_words(H, W))");
    return LA3D_ERR_ARG;
  }
  if ((long long)H * W > (1LL << 20)) {
    set_err("la3d_mask_stats_bits: the bit image must fit LDS (H*W <= 1048576)");
    return LA3D_ERR_UNSUPPORTED;
  }
  if (B == 0) return LA3D_SUCCESS;
  const int nwords = (int)la3d_mask_bits_words(H, W);
  const int vec = ((reinterpret_cast<uintptr_t>(bits) & 15) == 0 && bits_plane_stride % 4 == 0) ? 1 : 0;
  allow_big_lds(reinterpret_cast<const void*>(mask_stats_bits_kernel));
  hipLaunchKernelGGL(mask_stats_bits_kernel, dim3(B), dim3(256), (((size_t)nwords * 4 + 15) & ~(size_t)15) + 16, static_cast<hipStream_t>(stream),
                     bits, (long long)bits_plane_stride, vec, H, W, frame_width > 0 ? frame_width : W, nwords, boundary, stats);
  return check_launch("mask_stats_bits_kernel");
}

}  // extern "C"

// ---- annotations -> bit planes: the checks and launches of the four entries ---------------------------------------------------
namespace {
constexpr size_t ANN_LDS_MAX = 160 * 1024 - 256;

// uniform form: LA3D_ERR_ARG / LA3D_ERR_UNSUPPORTED, 1 = nothing to do (B == 0), LA3D_SUCCESS = launch
int ann_bits_check(const char* who, bool null_src, int B, int H, int W, int W_out, const uint32_t* bits, long long bits_plane_stride,
                   const int32_t* area) {
  char msg[240];
  const char* bad = nullptr;
  if (B < 0 || H <= 0 || W <= 0 || W_out < W) bad = "bad argument (B >= 0, H, W > 0, W_out >= W)";
  else if (W_out != W && W_out % 32 != 0) bad = "W_out must be W or a multiple of 32 (padded rows are whole words)";
  else if (B > 0 && (null_src || !bits)) bad = "NULL annotation arrays or bits";
  else if (B > 0 && ((reinterpret_cast<uintptr_t>(bits) | reinterpret_cast<uintptr_t>(area)) & 3)) bad = "bits or area not a 4-byte aligned pointer";
  if (!bad && (long long)H * W_out > (1LL << 20)) {   // (before the stride rule: its word count is then known to fit an int)
    snprintf(msg, sizeof(msg), "%s: the bit image must fit LDS (H*W_out <= 1048576)", who);
    set_err(msg);
    return LA3D_ERR_UNSUPPORTED;
  }
  if (!bad && B > 0 && bits_plane_stride < (long long)la3d_mask_bits_words(H, W_out)) bad = "bits_plane_stride is smaller than la3d_mask_bits_words(H, W_out)";
  if (bad) {
    snprintf(msg, sizeof(msg), "%s: %s", who, bad);
    set_err(msg);
    return LA3D_ERR_ARG;
  }
  return B == 0 ? 1 : LA3D_SUCCESS;
}

// frames form; *words_out: the words of the bounds' plane (rows of whole words)
int ann_bits_frames_check(const char* who, bool null_src, const la3d_frame* frames, int P, int H, int W, const int32_t* image_index, int B,
                          const uint32_t* bits, const int64_t* bits_offsets, const int32_t* area, long long* words_out) {
  char msg[240];
  const char* bad = nullptr;
  if (B < 0 || P < 0 || H <= 0 || W <= 0) bad = "bad argument (B, P >= 0, bounds H, W > 0)";
  else if (B > 0 && (null_src || (P > 0 && !frames) || !image_index || !bits || !bits_offsets))
    bad = "NULL annotation arrays, frames, image_index, bits or bits_offsets";
  else if (B > 0 && (reinterpret_cast<uintptr_t>(bits) & 15)) bad = "bits not a 16-byte aligned pointer";
  else if (B > 0 && ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(bits_offsets)) & 7))
    bad = "frames or bits_offsets not an 8-byte aligned pointer";
  else if (B > 0 && ((reinterpret_cast<uintptr_t>(image_index) | reinterpret_cast<uintptr_t>(area)) & 3))
    bad = "image_index or area not a 4-byte aligned pointer";
  if (bad) {
    snprintf(msg, sizeof(msg), "%s: %s", who, bad);
    set_err(msg);
    return LA3D_ERR_ARG;
  }
  const long long words = (long long)H * ((W + 31) / 32);
  if (words > (1LL << 15)) {
    snprintf(msg, sizeof(msg), "%s: the bit image of the bounds must fit LDS (H * roundup32(W) <= 1048576)", who);
    set_err(msg);
    return LA3D_ERR_UNSUPPORTED;
  }
  *words_out = words;
  return B == 0 ? 1 : LA3D_SUCCESS;
}

inline size_t rle_bits_lds(int lds_words, int scan_words) { return (size_t)lds_words * 4 + 64 + (size_t)scan_words * 4; }
inline size_t poly_bits_lds(int lds_words) { return (((size_t)lds_words * 4 + 15) & ~(size_t)15) + POLY_STAGE_BYTES + 64; }

int ann_lds_refuse(const char* who) {
  char msg[200];
  snprintf(msg, sizeof(msg), "%s: frame too large for LDS", who);
  set_err(msg);
  return LA3D_ERR_UNSUPPORTED;
}

BitsOut bits_out_uniform(int H, int W, int W_out, uint32_t* bits, long long stride, int32_t* area) {
  BitsOut c = {};
  c.bits = bits; c.stride = stride; c.area = area;
  c.H = H; c.W = W_out; c.frame_w = W_out > W ? W : 0;
  c.lds_words = (int)la3d_mask_bits_words(H, W_out);
  c.vec = ((reinterpret_cast<uintptr_t>(bits) & 15) == 0 && stride % 4 == 0) ? 1 : 0;
  return c;
}

BitsOut bits_out_frames(const la3d_frame* frames, int P, int H, int W, const int32_t* image_index, uint32_t* bits, const int64_t* bits_offsets,
                        int32_t* area, long long words) {
  BitsOut c = {};
  c.bits = bits; c.offsets = reinterpret_cast<const long long*>(bits_offsets); c.area = area;
  c.frames = frames; c.image_index = image_index; c.P = P;
  c.H = H; c.W = W; c.lds_words = (int)words; c.vec = 1;
  return c;
}
}  // namespace

extern "C" {

int la3d_pack_rle_bits(const int32_t* counts, const int64_t* offsets, int B, int H, int W, int W_out, uint32_t* bits,
                       int64_t bits_plane_stride, int32_t* area, void* stream) {
  const int rc = ann_bits_check("la3d_pack_rle_bits", !counts || !offsets, B, H, W, W_out, bits, bits_plane_stride, area);
  if (rc != LA3D_SUCCESS) return rc < 0 ? rc : LA3D_SUCCESS;
  const BitsOut c = bits_out_uniform(H, W, W_out, bits, bits_plane_stride, area);
  // (the block totals of the column scan, as in la3d_rle_decode: word-aligned rows only)
  const int ntx = W_out / 32;
  const int scan_words = (W_out % 32 == 0) ? ((NT_DEC / ntx > 2 ? NT_DEC / ntx : 2) * ntx) : 0;
  const size_t lds = rle_bits_lds(c.lds_words, scan_words);
  if (lds > ANN_LDS_MAX) return ann_lds_refuse("la3d_pack_rle_bits");
  allow_big_lds(reinterpret_cast<const void*>(pack_rle_bits_kernel<false>));
  hipLaunchKernelGGL(pack_rle_bits_kernel<false>, dim3(B), dim3(NT_DEC), lds, static_cast<hipStream_t>(stream), counts,
                     reinterpret_cast<const long long*>(offsets), scan_words, c);
  return check_launch("pack_rle_bits_kernel");
}

int la3d_pack_poly_bits(const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, int B, int H, int W, int W_out,
                        uint32_t* bits, int64_t bits_plane_stride, int32_t* area, void* stream) {
  const int rc = ann_bits_check("la3d_pack_poly_bits", !poly_xy || !ring_offsets || !inst_rings, B, H, W, W_out, bits, bits_plane_stride, area);
  if (rc != LA3D_SUCCESS) return rc < 0 ? rc : LA3D_SUCCESS;
  const BitsOut c = bits_out_uniform(H, W, W_out, bits, bits_plane_stride, area);
  const size_t lds = poly_bits_lds(c.lds_words);
  if (lds > ANN_LDS_MAX) return ann_lds_refuse("la3d_pack_poly_bits");
  allow_big_lds(reinterpret_cast<const void*>(pack_poly_bits_kernel<false>));
  hipLaunchKernelGGL(pack_poly_bits_kernel<false>, dim3(B), dim3(NT_DEC), lds, static_cast<hipStream_t>(stream), poly_xy,
                     reinterpret_cast<const long long*>(ring_offsets), reinterpret_cast<const long long*>(inst_rings), c);
  return check_launch("pack_poly_bits_kernel");
}

int la3d_pack_rle_bits_frames(const int32_t* counts, const int64_t* offsets, const la3d_frame* frames, int32_t P, int H, int W,
                              const int32_t* image_index, int B, uint32_t* bits, const int64_t* bits_offsets, int32_t* area,
                              void* stream) {
  long long words = 0;
  const int rc = ann_bits_frames_check("la3d_pack_rle_bits_frames", !counts || !offsets, frames, P, H, W, image_index, B, bits, bits_offsets,
                                       area, &words);
  if (rc != LA3D_SUCCESS) return rc < 0 ? rc : LA3D_SUCCESS;
  const BitsOut c = bits_out_frames(frames, P, H, W, image_index, bits, bits_offsets, area, words);
  // every frame of the call has at most (W + 31) / 32 words per row: room for two block rows of the widest, NT_DEC items otherwise
  const int ntx = (W + 31) / 32;
  const int scan_words = 2 * ntx > NT_DEC ? 2 * ntx : NT_DEC;
  const size_t lds = rle_bits_lds(c.lds_words, scan_words);
  if (lds > ANN_LDS_MAX) return ann_lds_refuse("la3d_pack_rle_bits_frames");
  allow_big_lds(reinterpret_cast<const void*>(pack_rle_bits_kernel<true>));
  hipLaunchKernelGGL(pack_rle_bits_kernel<true>, dim3(B), dim3(NT_DEC), lds, static_cast<hipStream_t>(stream), counts,
                     reinterpret_cast<const long long*>(offsets), scan_words, c);
  return check_launch("pack_rle_bits_frames_kernel");
}

int la3d_pack_poly_bits_frames(const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, const la3d_frame* frames,
                               int32_t P, int H, int W, const int32_t* image_index, int B, uint32_t* bits, const int64_t* bits_offsets,
                               int32_t* area, void* stream) {
  long long words = 0;
  const int rc = ann_bits_frames_check("la3d_pack_poly_bits_frames", !poly_xy || !ring_offsets || !inst_rings, frames, P, H, W, image_index, B,
                                       bits, bits_offsets, area, &words);
  if (rc != LA3D_SUCCESS) return rc < 0 ? rc : LA3D_SUCCESS;
  const BitsOut c = bits_out_frames(frames, P, H, W, image_index, bits, bits_offsets, area, words);
  const size_t lds = poly_bits_lds(c.lds_words);
  if (lds > ANN_LDS_MAX) return ann_lds_refuse("la3d_pack_poly_bits_frames");
  allow_big_lds(reinterpret_cast<const void*>(pack_poly_bits_kernel<true>));
  hipLaunchKernelGGL(pack_poly_bits_kernel<true>, dim3(B), dim3(NT_DEC), lds, static_cast<hipStream_t>(stream), poly_xy,
                     reinterpret_cast<const long long*>(ring_offsets), reinterpret_cast<const long long*>(inst_rings), c);
  return check_launch("pack_poly_bits_frames_kernel");
}

}  // extern "C"

// ---- masks as label maps ------------------------------------------------------------------
// include/la3d.h "masks as label maps": one (H, W) plane of segment ids per image -> one bit plane per (image, id) row, in the
// format of the packers above.  Both forms hold the 32 labels of an output word in registers and loop over the image's instances,
// so the labels of an image are read once however many instances it has.
namespace {
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
// stream it had: moved into this function its U16 / I32 loops schedule differently)
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
// before anything is read through it; so is a plane whose offset is negative or not a multiple of 4.  blockIdx.x = image * chunks +
// chunk, chunks sized for the bounds' plane: a chunk beyond its image's words returns before any load.
__device__ inline long long plane_offset(const long long* __restrict__ offs, int b) {
  const long long v = offs[b];
  return ((long long)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ inline unsigned image_columns(int w, int W, int fw) {
  const int rem = fw - (w % (W >> 5)) * 32;
  return rem >= 32 ? 0xffffffffu : rem <= 0 ? 0u : (1u << rem) - 1u;
}

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
  const FrameRow r = frame_row_load(frames + p);
  if (!frame_row_ok(r, max_h, max_w)) return;   // (uniform) a broken row: nothing is read through it, nothing written for it
  const int nwords = (r.H * r.W) >> 5;   // (<= the bounds' plane: H <= max_h, W <= max_w)
  if (chunk * 256 >= nwords) return;     // (uniform) a chunk beyond this image's words
  const int w = chunk * 256 + (int)threadIdx.x;
  const bool live = w < nwords;
  const unsigned have = live ? image_columns(w, r.W, r.fw) : 0u;
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
    const long long oo = plane_offset(out_offsets, b);
    if (oo < 0 || (oo & 3) != 0) continue;   // (uniform) before an address is formed from it: the fit refuses this instance too
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
  const FrameRow r = frame_row_load(frames + p);
  if (!frame_row_ok(r, max_h, max_w)) return;   // (uniform)
  const int nwords = (r.H * r.W) >> 5;
  if (chunk * 256 >= nwords) return;   // (uniform)
  const int w = chunk * 256 + (int)threadIdx.x;
  const bool live = w < nwords;
  const unsigned have = live ? image_columns(w, r.W, r.fw) : 0u;
  const unsigned char* sp = labels + (r.off + (long long)w * 32) * 3;   // (pixel 32 w of the plane: row w / (W/32), column 32 (w % (W/32)))
  int lab[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    lab[k] = 0;
    if ((have >> k) & 1u) lab[k] = (int)sp[k * 3] | (int)sp[k * 3 + 1] << 8 | (int)sp[k * 3 + 2] << 16;
  }
  for (int b = i0; b < i1; ++b) {   // uniform trip count
    const long long oo = plane_offset(out_offsets, b);
    if (oo < 0 || (oo & 3) != 0) continue;   // (uniform)
    const int id = inst_label[b];
    unsigned pat = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) pat |= (lab[k] == id ? 1u : 0u) << k;
    pat &= have;
    if (live) out[oo + w] = pat;
    label_area(area, b, pat);
  }
}

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
}  // namespace

extern "C" {

int la3d_pack_label_bits(const void* labels, int dtype, int64_t plane_stride, int P, int H, int W, int W_out,
                         const int32_t* inst_offsets, const int32_t* inst_label, int B, uint32_t* bits, int64_t bits_plane_stride,
                         int32_t* area, void* stream) {
  const char* bad = nullptr;
  const bool work = B > 0 && P > 0;
  if (dtype != LA3D_LABEL_U8 && dtype != LA3D_LABEL_U16 && dtype != LA3D_LABEL_I32 && dtype != LA3D_LABEL_RGB8)
    bad = "unknown dtype (LA3D_LABEL_U8, LA3D_LABEL_U16, LA3D_LABEL_I32 or LA3D_LABEL_RGB8)";
  else if (B < 0 || P < 0 || H <= 0 || W <= 0 || W_out < W) bad = "bad argument (B, P >= 0, H, W > 0, W_out >= W)";
  else if ((long long)H * W_out > (1LL << 28) || (long long)P * (((long long)H * W_out + 8191) / 8192) > 0x7fffffffLL)
    bad = "frame or batch too large (H*W_out <= 2^28, P * ceil(H*W_out / 8192) < 2^31)";
  else if (work && (!labels || !inst_offsets || !inst_label || !bits)) bad = "NULL labels, inst_offsets, inst_label or bits";
  else if (work && (reinterpret_cast<uintptr_t>(bits) & 3)) bad = "bits not a 4-byte aligned pointer";
  else if (work && (reinterpret_cast<uintptr_t>(labels) & (dtype == LA3D_LABEL_I32 ? 3 : dtype == LA3D_LABEL_U16 ? 1 : 0)))
    bad = "labels not aligned to their element size";
  else if (work && ((reinterpret_cast<uintptr_t>(inst_offsets) | reinterpret_cast<uintptr_t>(inst_label) | reinterpret_cast<uintptr_t>(area)) & 3))
    bad = "inst_offsets, inst_label or area not a 4-byte aligned pointer";
  else if (work && plane_stride < (long long)H * W) bad = "label plane stride smaller than H*W";
  else if (work && bits_plane_stride < (long long)la3d_mask_bits_words(H, W_out))
    bad = "bits_plane_stride is smaller than la3d_mask_bits_words(H, W_out)";
  if (bad) {
    char msg[200];
    snprintf(msg, sizeof(msg), "la3d_pack_label_bits: %s", bad);
    set_err(msg);
    return LA3D_ERR_ARG;
  }
  if (!work) return LA3D_SUCCESS;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (area) {   // cleared by a kernel of the call's own on the call's stream: a kernel node like the packer's when captured
    hipLaunchKernelGGL(clear_area_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, area, B);
    const int rc = check_launch("clear_area_kernel");
    if (rc != LA3D_SUCCESS) return rc;
  }
  switch (dtype) {
    case LA3D_LABEL_U8: return pack_labels_launch<LB_U8>(labels, plane_stride, P, H, W, W_out, inst_offsets, inst_label, B, bits, bits_plane_stride, area, s);
    case LA3D_LABEL_U16: return pack_labels_launch<LB_U16>(labels, plane_stride, P, H, W, W_out, inst_offsets, inst_label, B, bits, bits_plane_stride, area, s);
    case LA3D_LABEL_I32: return pack_labels_launch<LB_I32>(labels, plane_stride, P, H, W, W_out, inst_offsets, inst_label, B, bits, bits_plane_stride, area, s);
    default: return pack_labels_launch<LB_RGB8>(labels, plane_stride, P, H, W, W_out, inst_offsets, inst_label, B, bits, bits_plane_stride, area, s);
  }
}

int la3d_pack_label_bits_frames(const void* labels, int dtype, const la3d_frame* frames, int32_t P, int H, int W,
                                const int32_t* inst_offsets, const int32_t* inst_label, int B, uint32_t* bits,
                                const int64_t* bits_offsets, int32_t* area, void* stream) {
  const char* bad = nullptr;
  const bool work = B > 0 && P > 0;
  const long long words = H > 0 && W > 0 ? (long long)H * ((W + 31) / 32) : 0;   // the bounds' plane: rows of whole words
  if (dtype != LA3D_LABEL_U8 && dtype != LA3D_LABEL_U16 && dtype != LA3D_LABEL_I32 && dtype != LA3D_LABEL_RGB8)
    bad = "unknown dtype (LA3D_LABEL_U8, LA3D_LABEL_U16, LA3D_LABEL_I32 or LA3D_LABEL_RGB8)";
  else if (B < 0 || P < 0 || H <= 0 || W <= 0) bad = "bad argument (B, P >= 0, bounds H, W > 0)";
  else if (words > (1LL << 23) || (long long)P * ((words + 255) / 256) > 0x7fffffffLL)
    bad = "bounds or batch too large (H * roundup32(W) <= 2^28, P * ceil(H * roundup32(W) / 8192) < 2^31)";
  else if (work && (!labels || !frames || !inst_offsets || !inst_label || !bits || !bits_offsets))
    bad = "NULL labels, frames, inst_offsets, inst_label, bits or bits_offsets";
  else if (work && (reinterpret_cast<uintptr_t>(labels) & 15)) bad = "labels not a 16-byte aligned pointer";
  else if (work && (reinterpret_cast<uintptr_t>(bits) & 3)) bad = "bits not a 4-byte aligned pointer";
  else if (work && ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(bits_offsets)) & 7))
    bad = "frames or bits_offsets not an 8-byte aligned pointer";
  else if (work && ((reinterpret_cast<uintptr_t>(inst_offsets) | reinterpret_cast<uintptr_t>(inst_label) | reinterpret_cast<uintptr_t>(area)) & 3))
    bad = "inst_offsets, inst_label or area not a 4-byte aligned pointer";
  if (bad) {
    char msg[200];
    snprintf(msg, sizeof(msg), "la3d_pack_label_bits_frames: %s", bad);
    set_err(msg);
    return LA3D_ERR_ARG;
  }
  if (!work) return LA3D_SUCCESS;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (area) {   // (as la3d_pack_label_bits: a kernel node of the call's own when captured)
    hipLaunchKernelGGL(clear_area_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, area, B);
    const int rc = check_launch("clear_area_kernel");
    if (rc != LA3D_SUCCESS) return rc;
  }
  const int chunks = (int)((words + 255) / 256);
  const dim3 grid((unsigned)((long long)P * chunks));
  const long long* offs = reinterpret_cast<const long long*>(bits_offsets);
  switch (dtype) {
    case LA3D_LABEL_U8:
      hipLaunchKernelGGL(pack_labels_frames_vec_kernel<LB_U8>, grid, dim3(256), 0, s, labels, frames, H, W, chunks, inst_offsets, inst_label, B, bits, offs, area);
      break;
    case LA3D_LABEL_U16:
      hipLaunchKernelGGL(pack_labels_frames_vec_kernel<LB_U16>, grid, dim3(256), 0, s, labels, frames, H, W, chunks, inst_offsets, inst_label, B, bits, offs, area);
      break;
    case LA3D_LABEL_I32:
      hipLaunchKernelGGL(pack_labels_frames_vec_kernel<LB_I32>, grid, dim3(256), 0, s, labels, frames, H, W, chunks, inst_offsets, inst_label, B, bits, offs, area);
      break;
    default:
      hipLaunchKernelGGL(pack_labels_frames_rgb8_kernel, grid, dim3(256), 0, s, static_cast<const unsigned char*>(labels), frames, H, W, chunks, inst_offsets,
                         inst_label, B, bits, offs, area);
  }
  return check_launch("pack_labels_frames_kernel");
}

}  // extern "C"

namespace {
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
  const int img = __builtin_amdgcn_readfirstlane(image_index[n]);
  if ((unsigned)img >= (unsigned)P) return;   // (uniform) before the frame row is addressed
  const FrameRow r = frame_row_load(frames + img);
  if (!frame_row_ok(r, max_h, max_w)) return;   // (uniform) a broken row: nothing read, nothing written
  const long long oo = plane_offset(out_offsets, n);
  if (oo < 0 || (oo & 3) != 0) return;   // (uniform) before an address is formed from it: the fit refuses this instance too
  const int nwords = (r.H * r.W) >> 5;   // (<= the bounds' plane: H <= max_h, W <= max_w)
  if (chunk * 256 >= nwords) return;     // (uniform) a chunk beyond this instance's words
  const int w = chunk * 256 + (int)threadIdx.x;
  const bool live = w < nwords;
  const long long so = plane_offset(src_offsets, n);
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
    pat &= image_columns(w, r.W, r.fw);
    out[oo + w] = pat;
  }
  label_area(area, n, pat);   // (every lane of the wave takes part)
}

template <int KIND>
int pack_masks_frames_launch(const void* src, const la3d_frame* frames, int P, int H, int W, const int32_t* image_index,
                             const int64_t* src_offsets, const int32_t* src_pitch, int B, float thr, uint32_t* bits,
                             const int64_t* bits_offsets, int32_t* area, hipStream_t s, int chunks) {
  hipLaunchKernelGGL(pack_masks_frames_kernel<KIND>, dim3((unsigned)((long long)B * chunks)), dim3(256), 0, s, src, frames, P, H, W, chunks,
                     image_index, reinterpret_cast<const long long*>(src_offsets), src_pitch, thr, bits,
                     reinterpret_cast<const long long*>(bits_offsets), area);
  return check_launch("pack_masks_frames_kernel");
}

// the checks and the launch the two entries share; kind: PK_*
int pack_masks_frames(const char* who, const void* src, int kind, float thr, const la3d_frame* frames, int P, int H, int W,
                      const int32_t* image_index, const int64_t* src_offsets, const int32_t* src_pitch, int B, uint32_t* bits,
                      const int64_t* bits_offsets, int32_t* area, void* stream) {
  const char* bad = nullptr;
  const bool work = B > 0 && P > 0;
  const long long words = H > 0 && W > 0 ? (long long)H * ((W + 31) / 32) : 0;   // the bounds' plane: rows of whole words
  const long long chunks = (words + 255) / 256;
  if (B < 0 || P < 0 || H <= 0 || W <= 0) bad = "bad argument (B, P >= 0, bounds H, W > 0)";
  else if (words > (1LL << 23) || (long long)B * chunks > 0x7fffffffLL)
    bad = "bounds or batch too large (H * roundup32(W) <= 2^28, B * ceil(H * roundup32(W) / 8192) < 2^31)";
  else if (work && (!src || !frames || !image_index || !src_offsets || !bits || !bits_offsets))
    bad = "NULL source, frames, image_index, src_offsets, bits or bits_offsets";
  else if (work && (reinterpret_cast<uintptr_t>(src) & (kind == PK_F32 ? 3 : kind == PK_U8 ? 0 : 1))) bad = "source not aligned to its element size";
  else if (work && (reinterpret_cast<uintptr_t>(bits) & 3)) bad = "bits not a 4-byte aligned pointer";
  else if (work && ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(src_offsets) | reinterpret_cast<uintptr_t>(bits_offsets)) & 7))
    bad = "frames, src_offsets or bits_offsets not an 8-byte aligned pointer";
  else if (work && ((reinterpret_cast<uintptr_t>(image_index) | reinterpret_cast<uintptr_t>(src_pitch) | reinterpret_cast<uintptr_t>(area)) & 3))
    bad = "image_index, src_pitch or area not a 4-byte aligned pointer";
  if (bad) {
    char msg[240];
    snprintf(msg, sizeof(msg), "%s: %s", who, bad);
    set_err(msg);
    return LA3D_ERR_ARG;
  }
  if (!work) return LA3D_SUCCESS;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (area) {   // (as la3d_pack_label_bits: a kernel node of the call's own when captured)
    hipLaunchKernelGGL(clear_area_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, area, B);
    const int rc = check_launch("clear_area_kernel");
    if (rc != LA3D_SUCCESS) return rc;
  }
  const int c = (int)chunks;
  switch (kind) {
    case PK_U8: return pack_masks_frames_launch<PK_U8>(src, frames, P, H, W, image_index, src_offsets, src_pitch, B, thr, bits, bits_offsets, area, s, c);
    case PK_F32: return pack_masks_frames_launch<PK_F32>(src, frames, P, H, W, image_index, src_offsets, src_pitch, B, thr, bits, bits_offsets, area, s, c);
    case PK_F16: return pack_masks_frames_launch<PK_F16>(src, frames, P, H, W, image_index, src_offsets, src_pitch, B, thr, bits, bits_offsets, area, s, c);
    default: return pack_masks_frames_launch<PK_BF16>(src, frames, P, H, W, image_index, src_offsets, src_pitch, B, thr, bits, bits_offsets, area, s, c);
  }
}
}  // namespace

extern "C" {

int la3d_pack_mask_bits_frames(const uint8_t* mask, const la3d_frame* frames, int32_t P, int H, int W, const int32_t* image_index,
                               const int64_t* src_offsets, const int32_t* src_pitch, int B, uint32_t* bits, const int64_t* bits_offsets,
                               int32_t* area, void* stream) {
  return pack_masks_frames("la3d_pack_mask_bits_frames", mask, PK_U8, 0.0f, frames, P, H, W, image_index, src_offsets, src_pitch, B, bits,
                           bits_offsets, area, stream);
}

int la3d_pack_logits_bits_frames(const void* logits, int dtype, float threshold, const la3d_frame* frames, int32_t P, int H, int W,
                                 const int32_t* image_index, const int64_t* src_offsets, const int32_t* src_pitch, int B, uint32_t* bits,
                                 const int64_t* bits_offsets, int32_t* area, void* stream) {
  if (dtype != LA3D_DTYPE_F32 && dtype != LA3D_DTYPE_F16 && dtype != LA3D_DTYPE_BF16) {
    set_err("la3d_pack_logits_bits_frames: unknown dtype (LA3D_DTYPE_F32, LA3D_DTYPE_F16 or LA3D_DTYPE_BF16)");
    return LA3D_ERR_ARG;
  }
  const int kind = dtype == LA3D_DTYPE_F32 ? PK_F32 : dtype == LA3D_DTYPE_F16 ? PK_F16 : PK_BF16;
  return pack_masks_frames("la3d_pack_logits_bits_frames", logits, kind, threshold, frames, P, H, W, image_index, src_offsets, src_pitch, B,
                           bits, bits_offsets, area, stream);
}

}  // extern "C"
