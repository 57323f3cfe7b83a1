// la3d_open.hip - morphology on bit planes (include/la3d.h "morphology on bit planes"): la3d_open_bits and its frames form,
// la3d_open_bits_frames.  The checks of the two entries are written out here - their rank is theirs, not pack_check's; from
// la3d_bitplanes.hpp come the planes of a frames call and their locator (FramesPlanes, frames_source, frames_dest), the realigned word
// of an image row (plane_row_word), the in-place rule (planes_overlap) and the wording shared with the packers.
#include <cstdint>
#include <cstddef>

#include "la3d_bitplanes.hpp"

namespace {
// ---- morphology on bit planes ---------------------------------------------------------------
// include/la3d.h "morphology on bit planes": binary opening by a k x k square of the nearest x s upscale of a plane, with the area and
// the bounding rectangle of the result.  One workgroup per (band of R output rows, instance); R is a multiple of 32, so a band begins
// on a word of the output whatever W_out is and no two workgroups write one word.  In LDS every row is word-ALIGNED (nw words, lanes
// over the word column: consecutive banks, no conflicts whatever the row stride):
//   A  the source rows the band needs, realigned (funnel shift by (v*W) & 31) and spread to s bits per bit - ONE row per source row:
//      the s upscaled rows that repeat it are indexed, never stored
//   B  upscaled rows [r0 - r, r0 + R + r): the AND of the k rows around each (vertical erosion); then, in place, the horizontal
//      opening of each row (erosion and dilation along x are one function of a word and its two neighbours, since 2r <= 30 bits);
//      a row is owned by ONE wave, which reads all of it before it writes, so the pass needs no second buffer
//   the OR of k rows of B (vertical dilation) is the output word, formed in registers, counted for the statistics and stored.
// Rows and columns outside the image are zero (SciPy's border_value = 0): an erosion window that leaves the image holds its own
// centre, which is zero, so nothing beyond the zero rows of A and the masked last word is needed.
// FRAMES (la3d_open_bits_frames, images of different sizes): the same passes on a geometry formed per instance from its la3d_frame row
// (open_instance, all of it wave-uniform: SGPRs); ONE band plan per call, from the bounds - the grid has the bounds' bands for every
// instance and LDS is requested for the bounds, an instance uses its own words per row of it.
constexpr int OPEN_NT = 256;
struct OpenArgs {
  const unsigned* bits; long long stride;   // input planes, words apart
  int H, W, fw;                             // source rows, stored width, image columns
  long long nwords_in;                      // words of an input plane (nothing beyond is read)
  int k, s;
  unsigned* out; long long out_stride;      // NULL: statistics only
  int H_out, W_out, nw;                     // output rows, stored width; words of an aligned upscaled row = ceil(s*fw / 32)
  int nwords_out;                           // words of an output plane
  int R, nA, nbands, vec;                   // band rows; rows of A; bands per plane; 16-byte stores allowed
  int* partial;                             // [B][nbands][8] or NULL
  FramesPlanes fr;                          // frames form (H, W: the bounds of the table; the fields above that speak of a plane are then
};                                          // formed per instance, open_instance)

__device__ inline unsigned spread_bits(unsigned x, int s) {   // the low 32 / s bits of x, each repeated s times
  if (s == 4) {
    x = (x | (x << 12)) & 0x000F000Fu; x = (x | (x << 6)) & 0x03030303u; x = (x | (x << 3)) & 0x11111111u;
    return x * 15u;
  }
  if (s == 2) {
    x = (x | (x << 8)) & 0x00FF00FFu; x = (x | (x << 4)) & 0x0F0F0F0Fu; x = (x | (x << 2)) & 0x33333333u; x = (x | (x << 1)) & 0x55555555u;
    return x * 3u;
  }
  return x;
}

// word wc of the aligned, upscaled form of source row v (0 <= v < H, wc < nw): columns at and beyond fw are zero whatever the plane holds
__device__ inline unsigned open_source_word(const OpenArgs& a, const unsigned* __restrict__ plane, int v, int wc) {
  const int nb = 32 >> (a.s >> 1), c0 = wc * nb;       // 32 / s for s = 1, 2, 4
  return spread_bits(plane_row_word(plane, a.nwords_in, a.W, v, c0, min(nb, a.fw - c0)), a.s);
}

__device__ inline unsigned long long and_window(unsigned long long x, int k) {   // bit i = AND of bits i .. i + k - 1
  int w = 1;
  for (; 2 * w <= k; w *= 2) x &= x >> w;
  if (w < k) x &= x >> (k - w);
  return x;
}
__device__ inline unsigned long long or_window(unsigned long long x, int k) {    // bit i = OR of bits i - k + 1 .. i
  int w = 1;
  for (; 2 * w <= k; w *= 2) x |= x << w;
  if (w < k) x |= x << (k - w);
  return x;
}
// horizontal opening of the word `c` between its neighbours `l` (lower columns) and `r`: with e[i] = AND x[i .. i + k - 1] the erosion is
// e[c - r] and its dilation OR e[c - k + 1 .. c]; both windows stay inside the three words because k - 1 <= 30
__device__ inline unsigned open_row_word(unsigned l, unsigned c, unsigned r, int k) {
  const unsigned long long lo = and_window(((unsigned long long)c << 32) | l, k);   // valid for bits 0 .. 33
  const unsigned long long hi = and_window(((unsigned long long)r << 32) | c, k);   // columns 32 .. 65
  const unsigned long long e = (lo & 0xffffffffull) | (hi << 32);
  return (unsigned)(or_window(e, k) >> 32);
}

// item `it` of a (rows x n) grid as (row, column), stepped by the workgroup's size without a division per item
struct OpenItem {
  int it, row, col, drow, dcol;
  __device__ OpenItem(int tid, int n) : it(tid), row(tid / n), col(tid - (tid / n) * n), drow(OPEN_NT / n), dcol(OPEN_NT - (OPEN_NT / n) * n) {}
  __device__ void next(int n) {
    it += OPEN_NT; row += drow; col += dcol;
    if (col >= n) { col -= n; ++row; }
  }
};

// The plane geometry of instance b.  Uniform form: the argument block's own, planes a stride apart.  Frames form: formed here from the
// la3d_frame row of image_index[b] by the locator of la3d_bitplanes.hpp (frames_source, then frames_dest where planes are stored) -
// every value wave-uniform, checked before an address is formed from it.  The output plane is the one frame_table lays out for an
// image of (s * H, s * fw): pitch roundup32(s * fw), so its rows are whole words.  false: refused - nothing is read, nothing is written.
template <bool FRAMES>
__device__ inline bool open_instance(const OpenArgs& a, int b, OpenArgs* g, const unsigned** plane, unsigned** op) {
  if constexpr (FRAMES) {
    FramesWork f;
    if (!frames_source(a.fr, a.bits, a.H, a.W, b, &f)) return false;
    const int fw_out = a.s * f.r.fw, W_out = (fw_out + 31) & ~31, H_out = a.s * f.r.H;
    const int words_out = H_out * (W_out >> 5);          // (<= 2^23: the entry bounds s * H * roundup32(s * W) by 2^28)
    long long oo = 0;
    if (a.out && !frames_dest(a.fr, b, words_out, &oo)) return false;
    g->H = f.r.H; g->W = f.r.W; g->fw = f.r.fw; g->nwords_in = f.nwords;
    g->H_out = H_out; g->W_out = W_out; g->nw = W_out >> 5; g->nwords_out = words_out;
    g->vec = (W_out & 127) == 0;                         // (out is 16-byte aligned - checked on the host - and the offset a multiple of 4)
    *plane = a.bits + f.off;                             // (formed only now: after the last check)
    *op = a.out ? a.out + oo : nullptr;
  } else {
    *plane = a.bits + (long long)b * a.stride;
    *op = a.out ? a.out + (long long)b * a.out_stride : nullptr;
  }
  return true;
}

template <bool FRAMES>
__global__ __launch_bounds__(OPEN_NT) void open_bits_kernel(const OpenArgs call) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int red[5 * (OPEN_NT / 64)];
  const int tid = threadIdx.x, b = blockIdx.x / call.nbands, band = blockIdx.x - b * call.nbands;
  // frames form: the grid has the bands of the bounds; a workgroup of a refused instance, or whose band lies below its instance's last
  // row, ends here (uniform: before any barrier)
  OpenArgs own;
  const unsigned* plane;
  unsigned* op;
  if constexpr (FRAMES) {
    own = call;
    if (!open_instance<true>(call, b, &own, &plane, &op)) return;
    if (band * call.R >= own.H_out) return;
  } else {
    open_instance<false>(call, b, nullptr, &plane, &op);
  }
  const OpenArgs& a = FRAMES ? own : call;
  unsigned* A = reinterpret_cast<unsigned*>(smem);
  unsigned* Bv = A + (size_t)a.nA * a.nw;
  const int r = a.k >> 1, s = a.s, nw = a.nw, k = a.k;
  const int r0 = band * a.R;
  const int rows = min(a.R, a.H_out - r0);            // output rows of this band (>= 1)
  // floor((r0 - 2r) / s): the first source row of A (negative above the image)
  const int t0 = r0 - 2 * r;
  const int ls = s >> 1;                               // log2 s for s = 1, 2, 4: x >> ls is floor(x / s), negative x included
  const int vA0 = t0 >> ls;
  for (OpenItem i(tid, nw); i.it < a.nA * nw; i.next(nw)) {
    const int v = vA0 + i.row;
    A[i.it] = (v >= 0 && v < a.H) ? open_source_word(a, plane, v, i.col) : 0u;
  }
  __syncthreads();
  // vertical erosion: B row j is upscaled row V = r0 - r + j, the AND of upscaled rows V - r .. V + r = source rows floor((V - r) / s) ..
  // floor((V + r) / s); V - r >= r0 - 2r, so both lie in A
  const int nB = rows + 2 * r;
  for (OpenItem i(tid, nw); i.it < nB * nw; i.next(nw)) {
    const int lo = t0 + i.row, hi = lo + 2 * r;       // upscaled rows V - r, V + r
    const int a0 = (lo >> ls) - vA0, a1 = (hi >> ls) - vA0;
    const unsigned* col = A + i.col;
    unsigned x = ~0u;
#pragma unroll 4
    for (int q = a0; q <= a1; ++q) x &= col[q * nw];
    Bv[i.it] = x;
  }
  __syncthreads();
  // horizontal opening, in place: wave w owns rows w, w + 4, ..; it reads the whole row (nw <= 256 = four words per lane) before it
  // writes any of it
  if (k > 1) {
    const int lane = tid & 63, wave = tid >> 6;
    for (int j = wave; j < nB; j += OPEN_NT / 64) {
      unsigned* row = Bv + j * nw;
      unsigned res[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int wc = q * 64 + lane;
        res[q] = 0u;
        if (wc < nw) res[q] = open_row_word(wc > 0 ? row[wc - 1] : 0u, row[wc], wc + 1 < nw ? row[wc + 1] : 0u, k);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int wc = q * 64 + lane;
        if (wc < nw) row[wc] = res[q];
      }
    }
  }
  __syncthreads();
  // vertical dilation: the word (v, wc) of the opened band, v relative to r0; counted for the statistics as it is formed
  const int tail = s * a.fw - (nw - 1) * 32;          // image bits of the last word column (1 .. 32)
  const unsigned tail_mask = tail < 32 ? (1u << tail) - 1u : ~0u;
  int area = 0, ymin = 0x7fffffff, ymax = -1, xmin = 0x7fffffff, xmax = -1;
  auto word = [&](int v, int wc) -> unsigned {
    if (wc >= nw) return 0u;
    const unsigned* col = Bv + v * nw + wc;
    unsigned x = 0u;
#pragma unroll 8
    for (int q = 0; q < k; ++q) x |= col[q * nw];                // B rows of upscaled rows r0 + v - r .. r0 + v + r
    if (wc == nw - 1) x &= tail_mask;
    return x;
  };
  auto count = [&](int v, int wc, unsigned x) {
    if (!x) return;
    area += __popc(x);
    ymin = min(ymin, r0 + v); ymax = max(ymax, r0 + v);
    xmin = min(xmin, wc * 32 + __ffs((int)x) - 1); xmax = max(xmax, wc * 32 + 31 - __clz((int)x));
  };
  const bool aligned = (a.W_out & 31) == 0;           // (frames form: always)
  if (op && aligned && a.vec) {                        // rows of whole words, 16-byte stores: four words per thread
    const int wq = a.W_out >> 7;                       // (vec: W_out % 128 == 0)
    u32x4* o4 = reinterpret_cast<u32x4*>(op + (long long)r0 * (a.W_out >> 5));
    for (OpenItem i(tid, wq); i.it < rows * wq; i.next(wq)) {
      const int v = i.row, q = i.col, it = i.it;
      u32x4 x;
      x.x = word(v, 4 * q); x.y = word(v, 4 * q + 1); x.z = word(v, 4 * q + 2); x.w = word(v, 4 * q + 3);
      count(v, 4 * q, x.x); count(v, 4 * q + 1, x.y); count(v, 4 * q + 2, x.z); count(v, 4 * q + 3, x.w);
      o4[it] = x;
    }
  } else if (op && aligned) {                          // rows of whole words, word stores
    const int ww = a.W_out >> 5;
    unsigned* o = op + (long long)r0 * ww;
    for (OpenItem i(tid, ww); i.it < rows * ww; i.next(ww)) {
      const unsigned x = word(i.row, i.col);
      count(i.row, i.col, x);
      o[i.it] = x;
    }
  } else {
    // statistics over the aligned words; then (W_out % 32 != 0) the general form of the store: every word of the band's range of the
    // plane is gathered from the rows that cross it
    if (a.partial)
      for (OpenItem i(tid, nw); i.it < rows * nw; i.next(nw)) count(i.row, i.col, word(i.row, i.col));
    if (!FRAMES && op) {
      const long long bit0 = (long long)r0 * a.W_out;                       // a multiple of 32
      const int w0 = (int)(bit0 >> 5);
      const int w1 = (int)min((long long)a.nwords_out, (bit0 + (long long)a.R * a.W_out) >> 5);
      for (int j = w0 + tid; j < w1; j += OPEN_NT) {
        unsigned x = 0u;
        int g = (j - w0) * 32, filled = 0;                                  // bit of the band at which the next piece begins
        while (filled < 32) {
          const int v = g / a.W_out, col = g - v * a.W_out;
          if (v >= rows) break;                                             // past the plane's last row: the tail bits stay zero
          const int n = min(32 - filled, a.W_out - col);
          const int wc = col >> 5, sh = col & 31;
          unsigned p = word(v, wc) >> sh;
          if (sh && sh + n > 32) p |= word(v, wc + 1) << (32 - sh);
          if (n < 32) p &= (1u << n) - 1u;
          x |= p << filled;
          filled += n; g += n;
        }
        op[j] = x;
      }
    }
  }
  if (a.partial) {
    area = wave_sum_i(area); ymin = wave_min_i(ymin); ymax = wave_max_i(ymax); xmin = wave_min_i(xmin); xmax = wave_max_i(xmax);
    const int wave = tid >> 6;
    if ((tid & 63) == 0) { red[wave] = area; red[4 + wave] = ymin; red[8 + wave] = ymax; red[12 + wave] = xmin; red[16 + wave] = xmax; }
    __syncthreads();
    if (tid == 0) {
      int* p = a.partial + ((long long)b * a.nbands + band) * 8;
      p[0] = red[0] + red[1] + red[2] + red[3];
      p[1] = min(min(red[4], red[5]), min(red[6], red[7]));
      p[2] = max(max(red[8], red[9]), max(red[10], red[11]));
      p[3] = min(min(red[12], red[13]), min(red[14], red[15]));
      p[4] = max(max(red[16], red[17]), max(red[18], red[19]));
    }
  }
}

// the band records of one instance -> stats[b] = area, x, y, w, h (cv2.boundingRect of a binary image; 0, 0, 0, 0 when empty): one
// wave per instance, every band record has one writer and one reader - no atomics
__device__ inline void open_stats_reduce(const int* __restrict__ p, int nbands, int lane, int* __restrict__ o) {
  int area = 0, ymin = 0x7fffffff, ymax = -1, xmin = 0x7fffffff, xmax = -1;
  for (int i = lane; i < nbands; i += 64) {
    area += p[i * 8]; ymin = min(ymin, p[i * 8 + 1]); ymax = max(ymax, p[i * 8 + 2]);
    xmin = min(xmin, p[i * 8 + 3]); xmax = max(xmax, p[i * 8 + 4]);
  }
  area = wave_sum_i(area); ymin = wave_min_i(ymin); ymax = wave_max_i(ymax); xmin = wave_min_i(xmin); xmax = wave_max_i(xmax);
  if (lane == 0) {
    const bool any = area > 0;
    o[0] = area; o[1] = any ? xmin : 0; o[2] = any ? ymin : 0; o[3] = any ? xmax - xmin + 1 : 0; o[4] = any ? ymax - ymin + 1 : 0;
  }
}
__global__ __launch_bounds__(64) void open_bits_stats_kernel(const int* __restrict__ partial, int nbands, int* __restrict__ stats) {
  const int b = blockIdx.x;
  open_stats_reduce(partial + (long long)b * nbands * 8, nbands, threadIdx.x, stats + (long long)b * 5);
}
// frames form: the decision of open_bits_kernel<true> made again, then only the records the instance's own bands wrote in this call
// (the grid's further bands wrote none); a refused row gets -1, 0, 0, 0, 0
__global__ __launch_bounds__(64) void open_bits_frames_stats_kernel(const OpenArgs call, int* __restrict__ stats) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int* o = stats + (long long)b * 5;
  OpenArgs own = call;
  const unsigned* plane;
  unsigned* op;
  if (!open_instance<true>(call, b, &own, &plane, &op)) {
    if (lane < 5) o[lane] = lane ? 0 : -1;
    return;
  }
  open_stats_reduce(call.partial + (long long)b * call.nbands * 8, (own.H_out + call.R - 1) / call.R, lane, o);
}

// the band of one launch: 64 output rows where the two LDS images of such a band stay within 48 KiB (three workgroups per CU), else 32
// - the least a band can have (its first row has to begin on a word of the output)
struct OpenPlan { int R, nA, nbands; size_t lds; };
OpenPlan open_plan(int H_out, int nw, int k, int s) {
  const int r = k / 2;
  auto at = [&](int R) {
    OpenPlan p;
    p.R = R;
    p.nA = (R + 4 * r - 1 + s - 1) / s + 1;          // floor((t0 + R + 4r - 1) / s) - floor(t0 / s) + 1 at most
    p.nbands = (H_out + R - 1) / R;
    p.lds = (size_t)(p.nA + R + 2 * r) * nw * sizeof(unsigned);
    return p;
  };
  const OpenPlan p64 = at(64);
  return (H_out > 32 && p64.lds <= 48 * 1024) ? p64 : at(32);
}
}  // namespace

extern "C" {

size_t la3d_open_bits_workspace_bytes(int B, int H, int upscale) {
  if (B <= 0 || H <= 0 || upscale <= 0) return 0;
  return (size_t)B * (((size_t)H * (size_t)upscale + 31) / 32) * 8 * sizeof(int);   // one record per band of 32 rows: no plan has more
}

int la3d_open_bits(const uint32_t* bits, int64_t bits_plane_stride, int B, int H, int W, int frame_width, int k, int upscale,
                   uint32_t* out_bits, int64_t out_plane_stride, int W_out, int32_t* stats, void* workspace, void* stream) {
  const char* who = "la3d_open_bits";
  const int s = upscale;
  if (B < 0 || H <= 0 || W <= 0) return refuse(who, "bad argument (B >= 0, H, W > 0)");
  if (k < 1 || k > 31 || !(k & 1)) return refuse(who, "k must be odd and lie in 1 .. 31");
  if (s != 1 && s != 2 && s != 4) return refuse(who, "upscale must be 1, 2 or 4");
  if (frame_width <= 0 || frame_width > W) return refuse(who, "frame_width must lie in (0, W]");
  if (!out_bits && !stats) return refuse(who, "nothing to do: out_bits and stats are both NULL");
  if (out_bits && (long long)W_out < (long long)s * frame_width) return refuse(who, "W_out is smaller than upscale * frame_width");
  if (B == 0) return LA3D_SUCCESS;
  if (!bits || (stats && !workspace)) return refuse(who, "bits (and workspace, with stats) must not be NULL");
  if ((reinterpret_cast<uintptr_t>(bits) | reinterpret_cast<uintptr_t>(out_bits) | reinterpret_cast<uintptr_t>(stats) |
       reinterpret_cast<uintptr_t>(workspace)) & 3)
    return refuse(who, "bits, out_bits, stats or workspace not a 4-byte aligned pointer");
  if (!out_bits) W_out = s * frame_width;             // statistics only: the plane that is never stored
  if ((long long)s * frame_width > 8192) return refuse(who, "upscale * frame_width must not exceed 8192 (a band of rows lives in LDS)", LA3D_ERR_UNSUPPORTED);
  if ((long long)s * H > (1LL << 28) || (long long)s * H * W_out > (1LL << 28))
    return refuse(who, "upscale * H * W_out must not exceed 2^28", LA3D_ERR_UNSUPPORTED);
  const int H_out = s * H;
  const long long words_in = (long long)la3d_mask_bits_words(H, W), words_out = ((long long)H_out * W_out + 31) / 32;
  if (bits_plane_stride < words_in) return refuse(who, BITS_STRIDE);
  if (out_bits) {
    if (out_plane_stride < words_out) return refuse(who, "out_plane_stride is smaller than la3d_mask_bits_words(upscale * H, W_out)");
    // neighbouring bands read each other's halo: the call cannot work in place
    if (planes_overlap(bits, (uintptr_t)B * (uintptr_t)bits_plane_stride, out_bits, (uintptr_t)B * (uintptr_t)out_plane_stride))
      return refuse(who, "the input planes and the output planes overlap");
  }
  const int nw = (s * frame_width + 31) / 32;
  const OpenPlan p = open_plan(H_out, nw, k, s);
  if ((long long)B * p.nbands > 0x7fffffffLL) return refuse(who, "too many bands for one launch (B * bands > 2^31 - 1)", LA3D_ERR_UNSUPPORTED);
  OpenArgs a = {};
  a.bits = bits; a.stride = bits_plane_stride; a.H = H; a.W = W; a.fw = frame_width; a.nwords_in = words_in;
  a.k = k; a.s = s; a.out = out_bits; a.out_stride = out_plane_stride;
  a.H_out = H_out; a.W_out = W_out; a.nw = nw; a.nwords_out = (int)words_out;
  a.R = p.R; a.nA = p.nA; a.nbands = p.nbands;
  a.vec = (out_bits && W_out % 128 == 0 && (reinterpret_cast<uintptr_t>(out_bits) & 15) == 0 && out_plane_stride % 4 == 0) ? 1 : 0;
  a.partial = stats ? static_cast<int*>(workspace) : nullptr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  allow_big_lds(reinterpret_cast<const void*>(open_bits_kernel<false>));
  hipLaunchKernelGGL(open_bits_kernel<false>, dim3((unsigned)((long long)B * p.nbands)), dim3(OPEN_NT), p.lds, st, a);
  const int rc = check_launch("open_bits_kernel");
  if (rc != LA3D_SUCCESS || !stats) return rc;
  hipLaunchKernelGGL(open_bits_stats_kernel, dim3((unsigned)B), dim3(64), 0, st, a.partial, p.nbands, stats);
  return check_launch("open_bits_stats_kernel");
}

size_t la3d_open_bits_frames_workspace_bytes(int B, int H, int upscale) { return la3d_open_bits_workspace_bytes(B, H, upscale); }

int la3d_open_bits_frames(const uint32_t* bits, int64_t bits_words, const int64_t* bits_offsets, const la3d_frame* frames, int32_t P, int H,
                          int W, const int32_t* image_index, int B, int k, int upscale, uint32_t* out_bits, int64_t out_words,
                          const int64_t* out_offsets, int32_t* stats, void* workspace, void* stream) {
  const char* who = "la3d_open_bits_frames";
  const int s = upscale;
  if (B < 0 || P < 0 || H <= 0 || W <= 0) return refuse(who, SIZES_FRAMES);
  if (k < 1 || k > 31 || !(k & 1)) return refuse(who, "k must be odd and lie in 1 .. 31");
  if (s != 1 && s != 2 && s != 4) return refuse(who, "upscale must be 1, 2 or 4");
  if (!out_bits && !stats) return refuse(who, "nothing to do: out_bits and stats are both NULL");
  if (bits_words < 0 || (out_bits && out_words < 0)) return refuse(who, "bits_words and out_words must not be negative");
  if (B > 0) {
    if (!bits || !bits_offsets || (!frames && P > 0) || !image_index) return refuse(who, "NULL bits, bits_offsets, frames or image_index");
    if (out_bits && !out_offsets) return refuse(who, "out_offsets must not be NULL with out_bits");
    if (stats && !workspace) return refuse(who, "workspace must not be NULL with stats");
  }
  if ((at(bits) | at(out_bits)) & 15) return refuse(who, "bits or out_bits not a 16-byte aligned pointer");
  if ((at(bits_offsets) | at(out_offsets) | at(frames)) & 7) return refuse(who, "bits_offsets, out_offsets or frames not an 8-byte aligned pointer");
  if ((at(stats) | at(workspace) | at(image_index)) & 3) return refuse(who, "stats, workspace or image_index not a 4-byte aligned pointer");
  // neighbouring bands read each other's halo: the call cannot work in place
  if (bits && out_bits && planes_overlap(bits, (uintptr_t)bits_words, out_bits, (uintptr_t)out_words))
    return refuse(who, "the input buffer and the output buffer overlap");
  if ((long long)s * W > 8192) return refuse(who, "upscale * W must not exceed 8192 (a band of rows lives in LDS)", LA3D_ERR_UNSUPPORTED);
  const long long W_out = ((long long)s * W + 31) / 32 * 32;
  if ((long long)s * H > (1LL << 28) || (long long)s * H * W_out > (1LL << 28))
    return refuse(who, "upscale * H * roundup32(upscale * W) must not exceed 2^28", LA3D_ERR_UNSUPPORTED);
  const OpenPlan p = open_plan(s * H, (int)(W_out / 32), k, s);   // one plan per call, from the bounds
  if ((long long)B * p.nbands > 0x7fffffffLL) return refuse(who, "too many bands for one launch (B * bands > 2^31 - 1)", LA3D_ERR_UNSUPPORTED);
  if (B == 0) return LA3D_SUCCESS;
  OpenArgs a = {};
  a.bits = bits; a.H = H; a.W = W; a.k = k; a.s = s; a.out = out_bits;
  a.R = p.R; a.nA = p.nA; a.nbands = p.nbands;
  a.partial = stats ? static_cast<int*>(workspace) : nullptr;
  a.fr.offsets = reinterpret_cast<const long long*>(bits_offsets); a.fr.out_offsets = reinterpret_cast<const long long*>(out_offsets);
  a.fr.frames = frames; a.fr.image_index = image_index; a.fr.P = P; a.fr.bits_words = bits_words; a.fr.out_words = out_bits ? out_words : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (P > 0) {   // (no image: every row is refused, which the statistics kernel alone says)
    allow_big_lds(reinterpret_cast<const void*>(open_bits_kernel<true>));
    hipLaunchKernelGGL(open_bits_kernel<true>, dim3((unsigned)((long long)B * p.nbands)), dim3(OPEN_NT), p.lds, st, a);
    const int rc = check_launch("open_bits_kernel");
    if (rc != LA3D_SUCCESS) return rc;
  }
  if (!stats) return LA3D_SUCCESS;
  hipLaunchKernelGGL(open_bits_frames_stats_kernel, dim3((unsigned)B), dim3(64), 0, st, a, stats);
  return check_launch("open_bits_frames_stats_kernel");
}

}  // extern "C"
