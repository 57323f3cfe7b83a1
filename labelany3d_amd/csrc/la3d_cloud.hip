// la3d_cloud.hip - instance point clouds (include/la3d.h "instance point clouds"): the masked, back-projected pixels of every instance,
//     points[offsets[n] + r] = depth_to_points(depth[img(n)][None], K[img(n)])[mask[n]][r]        # src/util.py:52-75, :480-481
// in two stages on the caller's stream, neither of which synchronises.
//   count + offsets   one workgroup per (instance, band of rows) turns its band of the mask into a bit image in LDS and counts it;
//                     the per-band counts stay in the workspace.  One workgroup then scans them: per instance the exclusive prefix
//                     over its bands (the rank at which a band starts), counts[B], and the exclusive prefix offsets[B+1] over the
//                     rows the instances occupy (the reference's 500-row rule with sample_idx, src/util_3dbox.py:123).
//   gather            the same grid builds the same bit image, scans the popcounts of its 64-pixel words in LDS and then works by
//                     OUTPUT ROW: the lane that owns rank q finds its pixel by select (binary search over the word prefix, then the
//                     q-th set bit of the word), so every lane of a step has a point to compute and a wave writes 64 consecutive rows.
//                     No atomics order anything: the rank of a pixel is workspace prefix + LDS prefix + bit position.
// The arithmetic of a point is unproject_frame's (la3d_masks.hip), term for term, behind the same in-kernel inv3 of K.
#include <cstdint>
#include <cstddef>
#include <cstring>

#include "la3d_bitplanes.hpp"   // (frames_prologue)
#include "la3d_point.hpp"

namespace {
constexpr int CT = 256;                     // threads per workgroup
constexpr int BAND_PIX = 65536;             // pixels (pitch x rows) a band holds at most: its bit image is 8 KiB of LDS
constexpr int BAND_WORDS = BAND_PIX / 64;   // 64-pixel words of a band
constexpr int MAX_BANDS = 64;               // bands per instance for parallelism (more only where BAND_PIX asks for them)
constexpr int WANT_WGS = 8192;              // workgroups a batch is spread over where its frames allow: four rounds of the resident set
                                            // (a band's work is a serial chain of select -> load -> store steps: short chains, many of them)

struct CloudParams {
  int B, H, W, fw, nb, P;
  int k_stride, d16_hole;
  float d16_scale;
  const void* depth; long long depth_stride;             // elements
  const int* image_index;
  const unsigned char* mask; long long mask_stride;      // bytes
  const unsigned* bits; long long bits_stride;           // words
  const long long* bits_offsets;
  const double* K;
  const int* sample_idx;
  const la3d_frame* frames;
  int* counts; long long* offsets;
  void* points; int* pixels; int* status; long long capacity;
  int* ws;                                               // [B][nb + 1]
};

// what a workgroup knows of its instance (wave-uniform)
struct CloudGeom {
  bool ok;
  int H, W, fw, img;
  long long depth_off;          // elements from the depth base to the instance's plane
  const unsigned char* mask;    // u8 plane, or null
  const unsigned* bits;         // bit plane (pitch W), or null
  long long plane_words;        // words of the bit plane
};

// Frames form: the decision is made before any address is formed from the row, by frames_prologue (image index, frame row, plane
// offset; la3d_bitplanes.hpp).  The entry has no length of the bit buffer, so there is no end check here.
template <bool FRAMES>
__device__ inline CloudGeom cloud_geom(const CloudParams& p, int n) {
  CloudGeom g;
  g.ok = false; g.mask = nullptr; g.bits = nullptr; g.plane_words = 0; g.depth_off = 0;
  g.H = p.H; g.W = p.W; g.fw = p.fw;
  g.img = __builtin_amdgcn_readfirstlane(p.image_index ? p.image_index[n] : n);
  if (FRAMES) {
    FramesWork f;
    if (!frames_prologue<true, false>(p.frames, p.P, p.image_index, p.H, p.W, const_cast<unsigned*>(p.bits), p.bits_offsets, n, 0, &f)) return g;
    g.H = f.r.H; g.W = f.r.W; g.fw = f.r.fw;
    g.depth_off = f.r.off;
    g.bits = f.out;
    g.plane_words = f.nwords;                      // (W % 32 == 0: whole words)
  } else {
    g.depth_off = (long long)g.img * p.depth_stride;
    if (p.mask) g.mask = p.mask + (long long)n * p.mask_stride;
    else {
      g.bits = p.bits + (long long)n * p.bits_stride;
      g.plane_words = ((long long)p.H * p.W + 31) >> 5;
    }
  }
  g.ok = true;
  return g;
}

struct CloudLds {
  unsigned long long words[BAND_WORDS];   // bit j of the band (pixel v0 * W + j of the plane) = bit j & 63 of word j >> 6
  unsigned pre[BAND_WORDS + 1];           // exclusive popcount prefix of the words; pre[BAND_WORDS] = the band's count
  unsigned short gw[BAND_WORDS];          // the word that holds rank 64 g, for every g with 64 g < the band's count: where a select starts
  unsigned wsum[CT / 64];
};

// Rows [v0, v1) of the instance's mask -> the band's bit image, columns >= frame width cleared, and its word prefix.  Returns the
// number of set pixels.  (v1 - v0) * W <= BAND_PIX.  Every thread of the workgroup calls it.
__device__ inline unsigned band_bits(const CloudGeom& g, int v0, int v1, CloudLds& L, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int npx = (v1 - v0) * g.W;
  const int nw64 = (npx + 63) >> 6;
  const long long p0 = (long long)v0 * g.W;
  if (g.mask) {
    const unsigned char* mp = g.mask + p0;
    if ((reinterpret_cast<uintptr_t>(mp) & 15) == 0 && (npx & 15) == 0) {   // the 16-byte form: 16 pixels per thread and step
      unsigned short* b16 = reinterpret_cast<unsigned short*>(L.words);
      const int n16 = npx >> 4;
#pragma unroll 4
      for (int c = tid; c < nw64 * 4; c += CT) {
        unsigned b = 0;
        if (c < n16) {
          const uint4 q = reinterpret_cast<const uint4*>(mp)[c];
          b = nz4(q.x) | (nz4(q.y) << 4) | (nz4(q.z) << 8) | (nz4(q.w) << 12);
        }
        b16[c] = (unsigned short)b;
      }
    } else {                                                                // the general form: one pixel per lane, one ballot per word
      for (int w = wave; w < nw64; w += CT / 64) {
        const int j = w * 64 + lane;
        const bool on = j < npx && mp[j] != 0;
        const unsigned long long bal = __ballot(on);
        if (lane == 0) L.words[w] = bal;
      }
    }
  } else {                                                                  // bit planes: one 32-bit word of the band per thread and step
    unsigned* b32 = reinterpret_cast<unsigned*>(L.words);
#pragma unroll 4
    for (int k = tid; k < nw64 * 2; k += CT) {
      unsigned val = 0;
      const int left = npx - 32 * k;
      if (left > 0) {
        const long long s = p0 + 32LL * k;
        const long long wi = s >> 5;
        const int sh = (int)(s & 31);
        val = g.bits[wi] >> sh;
        if (sh != 0 && wi + 1 < g.plane_words) val |= g.bits[wi + 1] << (32 - sh);
        if (left < 32) val &= (1u << left) - 1u;
      }
      b32[k] = val;
    }
  }
  __syncthreads();
  if (g.fw < g.W) {   // padded rows: whatever the planes hold beyond the image columns is no pixel
    unsigned* b32 = reinterpret_cast<unsigned*>(L.words);
    const int wpp = ((g.W - g.fw + 31) >> 5) + 1;   // 32-bit words the padding of one row can touch
    const int rows = v1 - v0;
    for (int idx = tid; idx < rows * wpp; idx += CT) {
      const int r = idx / wpp, k = idx - r * wpp;
      const int lo = r * g.W + g.fw, hi = (r + 1) * g.W;
      const int wd = (lo >> 5) + k;
      const int a = max(lo, wd * 32), b = min(hi, wd * 32 + 32);
      if (a < b) {
        const unsigned m = (b - a == 32) ? 0xffffffffu : (((1u << (b - a)) - 1u) << (a - wd * 32));
        atomicAnd(&b32[wd], ~m);
      }
    }
    __syncthreads();
  }
  // popcounts of the words and their exclusive prefix: four consecutive words per thread, a shuffle scan per wave, the wave sums in LDS
  unsigned c[4], s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int w = tid * 4 + i;
    c[i] = w < nw64 ? (unsigned)__popcll(L.words[w]) : 0u;
    s += c[i];
  }
  unsigned inc = s;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) L.wsum[wave] = inc;
  __syncthreads();
  unsigned run = inc - s;
  for (int i = 0; i < wave; ++i) run += L.wsum[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    L.pre[tid * 4 + i] = run;
    // a word holds at most 64 ranks, so at most one multiple of 64 among them
    const unsigned g = (run + 63u) >> 6;
    if ((g << 6) < run + c[i]) L.gw[g] = (unsigned short)(tid * 4 + i);
    run += c[i];
  }
  if (tid == CT - 1) L.pre[BAND_WORDS] = run;
  __syncthreads();
  return L.pre[BAND_WORDS];
}

// the k-th (from 0) set bit of x; k < popcount(x)
__device__ inline int select64(unsigned long long x, unsigned k) {
  int pos = 0;
  unsigned y = (unsigned)x;
  unsigned c = (unsigned)__popc(y);
  if (k >= c) { k -= c; pos = 32; y = (unsigned)(x >> 32); }
#pragma unroll
  for (int w = 16; w >= 1; w >>= 1) {
    const unsigned lowmask = (1u << w) - 1u;
    c = (unsigned)__popc(y & lowmask);
    if (k >= c) { k -= c; pos += w; y >>= w; }
    y &= lowmask;
  }
  return pos;
}

// the band-relative pixel of band-local rank q (q < total, the band's count): the search runs between the words that hold the first
// rank of q's group of 64 and the first rank of the next group - one or two words in a filled region
__device__ inline int band_select(const CloudLds& L, unsigned q, int nw64, unsigned total) {
  const unsigned g = q >> 6;
  int lo = L.gw[g], hi = (((g + 1u) << 6) < total) ? (int)L.gw[g + 1] + 1 : nw64;   // pre[lo] <= q < pre[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (L.pre[mid] <= q) lo = mid; else hi = mid;
  }
  return lo * 64 + select64(L.words[lo], q - L.pre[lo]);
}

// a point of the cloud: cloud_point (la3d_point.hpp), shared with the ground plane's sample select

__device__ inline void band_rows(const CloudGeom& g, int nb, int band, int* v0, int* v1) {
  const int rpb = (g.H + nb - 1) / nb;
  *v0 = band * rpb;
  *v1 = min(g.H, *v0 + rpb);
}

// ---- stage 1 ------------------------------------------------------------------------------------------------------------
template <bool FRAMES>
__global__ __launch_bounds__(CT) void cloud_count_kernel(const CloudParams p) {
  __shared__ CloudLds L;
  const int n = blockIdx.x / p.nb, band = blockIdx.x - n * p.nb;
  const CloudGeom g = cloud_geom<FRAMES>(p, n);
  unsigned total = 0;
  if (g.ok) {
    int v0, v1;
    band_rows(g, p.nb, band, &v0, &v1);
    if (v0 < v1) total = band_bits(g, v0, v1, L, threadIdx.x);
  }
  if (threadIdx.x == 0) p.ws[(long long)n * (p.nb + 1) + band] = (int)total;
}

// One workgroup: per instance the band counts become band prefixes (ws[n][nb] = N_n), counts[n] = N_n, and offsets = the exclusive
// prefix of the rows.  Thread t owns a run of consecutive instances, the runs are scanned in LDS: deterministic, any B.
constexpr int ST = 1024;
__global__ __launch_bounds__(ST) void cloud_scan_kernel(const CloudParams p) {
  __shared__ long long part[ST];
  const int tid = threadIdx.x;
  const int chunk = (p.B + ST - 1) / ST;
  const int n0 = min(p.B, tid * chunk), n1 = min(p.B, n0 + chunk);
  long long sum = 0;
  for (int n = n0; n < n1; ++n) {
    int* w = p.ws + (long long)n * (p.nb + 1);
    int run = 0;
    for (int b = 0; b < p.nb; ++b) {
      const int c = w[b];
      w[b] = run;
      run += c;
    }
    w[p.nb] = run;
    p.counts[n] = run;
    const int rows = (p.sample_idx && run > LA3D_NSAMPLE) ? LA3D_NSAMPLE : run;
    p.offsets[n + 1] = rows;   // (replaced by the prefix below, by this thread)
    sum += rows;
  }
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < ST; d <<= 1) {
    const long long t = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += t;
    __syncthreads();
  }
  long long run = part[tid] - sum;
  if (tid == 0) p.offsets[0] = 0;
  for (int n = n0; n < n1; ++n) {
    run += p.offsets[n + 1];
    p.offsets[n + 1] = run;
  }
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------------
// status of every instance before its bands run: one wave per instance
template <bool FRAMES>
__global__ __launch_bounds__(CT) void cloud_status_kernel(const CloudParams p) {
  const int n = blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
  if (n >= p.B) return;
  const CloudGeom g = cloud_geom<FRAMES>(p, n);
  int st = LA3D_CLOUD_OK;
  if (!g.ok) st = LA3D_BOX_UNSUPPORTED;
  else {
    const long long off0 = p.offsets[n], off1 = p.offsets[n + 1];
    if (off0 < 0 || off1 < off0 || off1 > p.capacity) st = LA3D_CLOUD_NO_ROOM;
    else {
      const int N = p.ws[(long long)n * (p.nb + 1) + p.nb];
      const int expect = (p.sample_idx && N > LA3D_NSAMPLE) ? LA3D_NSAMPLE : N;
      if (off1 - off0 != expect) st = LA3D_CLOUD_MISMATCH;
    }
  }
  if ((threadIdx.x & 63) == 0) p.status[n] = st;
}

template <typename DT, typename OutT, bool FRAMES>
__global__ __launch_bounds__(CT) void cloud_gather_kernel(const CloudParams p, const DepthCvt<DT> cv) {
  __shared__ CloudLds L;
  __shared__ double kinv[9];
  __shared__ __attribute__((aligned(16))) OutT stage[CT / 64][192];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x / p.nb, band = blockIdx.x - n * p.nb;
  const CloudGeom g = cloud_geom<FRAMES>(p, n);
  if (!g.ok) return;                                                     // (status 5, nothing written)
  const long long off0 = p.offsets[n], off1 = p.offsets[n + 1];
  if (off0 < 0 || off1 < off0 || off1 > p.capacity) return;              // (status 1, nothing written)
  const long long len = off1 - off0;
  int v0, v1;
  band_rows(g, p.nb, band, &v0, &v1);
  if (v0 >= v1) return;
  const int* wsn = p.ws + (long long)n * (p.nb + 1);
  const int bp = wsn[band], wcnt = wsn[band + 1] - bp, N = wsn[p.nb];    // what the offsets stage counted
  if (tid == 0) inv3(p.K + (long long)g.img * p.k_stride, kinv);
  const int actual = (int)band_bits(g, v0, v1, L, tid);
  if (actual != wcnt || bp < 0) {                                        // the masks changed between the two calls
    if (tid == 0) atomicMax(p.status + n, LA3D_CLOUD_MISMATCH);
    if (bp < 0 || wcnt < 0) return;
  }
  const int nw64 = ((v1 - v0) * g.W + 63) >> 6;
  const DT* dp = static_cast<const DT*>(p.depth) + g.depth_off + (long long)v0 * g.W;
  const float rcpW = 1.0f / (float)g.W;
  OutT* pts = static_cast<OutT*>(p.points) + off0 * 3;
  int* pix = p.pixels ? p.pixels + off0 : nullptr;
  const int have = min(actual, wcnt);   // ranks of this band that exist AND were given rows
  if (!(p.sample_idx && N > LA3D_NSAMPLE)) {
    // rows bp .. bp + have of the instance, as far as its range reaches
    const long long room = len - bp;
    const int nq = (int)(room < have ? (room < 0 ? 0 : room) : have);
    OutT* sl = stage[wave];
    for (int t0 = wave * 64; t0 < nq; t0 += CT) {   // wave-uniform trip count
      const int q = t0 + lane;
      double w[3] = {0, 0, 0};
      int pixel = -1;
      if (q < nq) {
        const int j = band_select(L, (unsigned)q, nw64, (unsigned)actual);
        unsigned u, dv;
        pix_uv((unsigned)j, g.W, rcpW, &u, &dv);
        cloud_point((double)depth_at<DT>(dp, j, cv), u, (unsigned)v0 + dv, kinv, w);
        pixel = (v0 + (int)dv) * g.fw + (int)u;
      }
      sl[lane * 3] = (OutT)w[0]; sl[lane * 3 + 1] = (OutT)w[1]; sl[lane * 3 + 2] = (OutT)w[2];
      // (lanes exchange through LDS: see unproject_frame)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int nv = min(64, nq - t0);
      OutT* op = pts + (long long)(bp + t0) * 3;
      if (nv == 64 && (reinterpret_cast<uintptr_t>(op) & 15) == 0) {   // uniform: 64 consecutive rows as whole 16-byte stores
        constexpr int N16 = 64 * 3 * (int)sizeof(OutT) / 16;
        const u32x4* s16 = reinterpret_cast<const u32x4*>(sl);
        u32x4* o16 = reinterpret_cast<u32x4*>(op);
#pragma unroll
        for (int k = 0; k < (N16 + 63) / 64; ++k)
          if (k * 64 + lane < N16) __builtin_nontemporal_store(s16[k * 64 + lane], o16 + k * 64 + lane);
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (k * 64 + lane < nv * 3) __builtin_nontemporal_store(sl[k * 64 + lane], op + k * 64 + lane);
      }
      if (pix && q < nq) __builtin_nontemporal_store(pixel, pix + bp + q);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  } else {
    // reference-subsample mode: row j of the instance = the point of rank sample_idx[n][j]; the band that holds the rank writes the
    // row, band 0 the NaN row of a rank outside [0, N)
    const int* si = p.sample_idx + (long long)n * LA3D_NSAMPLE;
    for (int j = tid; j < LA3D_NSAMPLE && j < len; j += CT) {
      const int r = si[j];
      double w[3];
      int pixel = -1;
      if (r < 0 || r >= N) {
        if (band != 0) continue;
        w[0] = w[1] = w[2] = __longlong_as_double(0x7ff8000000000000LL);
      } else {
        const int q = r - bp;
        if (q < 0 || q >= have) continue;
        const int px = band_select(L, (unsigned)q, nw64, (unsigned)actual);
        unsigned u, dv;
        pix_uv((unsigned)px, g.W, rcpW, &u, &dv);
        cloud_point((double)depth_at<DT>(dp, px, cv), u, (unsigned)v0 + dv, kinv, w);
        pixel = (v0 + (int)dv) * g.fw + (int)u;
      }
      OutT* op = pts + (long long)j * 3;
      op[0] = (OutT)w[0]; op[1] = (OutT)w[1]; op[2] = (OutT)w[2];
      if (pix) pix[j] = pixel;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// bands per instance: enough for the parallelism of a small batch, and never fewer than BAND_PIX asks for
int cloud_bands(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || W > BAND_PIX) return 0;
  const int rows_max = BAND_PIX / W;                 // rows a band may hold
  int nb = (H + rows_max - 1) / rows_max;            // smallest count that fits
  int par = (WANT_WGS + B - 1) / B;
  if (par > MAX_BANDS) par = MAX_BANDS;
  if (par > (H + 3) / 4) par = (H + 3) / 4;          // (no band below four rows for parallelism's sake)
  if (nb < par) nb = par;
  return nb;
}

// the checks of both entries, made before any launch; on success `p` is the kernel argument and `a` the caller's block with the
// fields it lacks zeroed
int cloud_check(const la3d_cloud_args* args, const char* who, bool gather, la3d_cloud_args& a, CloudParams& p) {
  static_assert(sizeof(la3d_cloud_args) == 192, "la3d_cloud_args is part of the ABI");
  if (!args || args->struct_size < (int32_t)sizeof(la3d_cloud_args)) return refuse(who, "bad struct_size");
  memcpy(&a, args, sizeof(a));   // (a longer block from a newer caller is fine)
  if (a.B < 0 || a.H < 0 || a.W < 0 || a.P < 0 || (a.B > 0 && (a.H == 0 || a.W == 0))) return refuse(who, "negative or empty sizes (B, H, W, P)");
  if (a.frame_width < 0 || a.frame_width > a.W) return refuse(who, "frame_width outside [0, W]");
  if (a.B == 0) {
    if (!gather && !a.offsets) return refuse(who, "offsets is NULL");
    memset(&p, 0, sizeof(p));
    p.offsets = reinterpret_cast<long long*>(a.offsets);
    return LA3D_SUCCESS;
  }
  if ((a.mask ? 1 : 0) + (a.mask_bits ? 1 : 0) != 1) return refuse(who, "give exactly one of mask / mask_bits");
  if ((a.depth ? 1 : 0) + (a.depth16 ? 1 : 0) != 1) return refuse(who, "give exactly one of depth / depth16");
  float d16_scale = 1.0f;
  int d16_hole = 0;
  const void* dplanes = a.depth;
  long long dstride = a.depth_plane_stride;
  if (a.depth16) {
    const la3d_depth16* d = a.depth16;
    if (d->struct_size < (int32_t)sizeof(la3d_depth16)) return refuse(who, "bad struct_size of la3d_depth16");
    if (d->dtype != LA3D_DTYPE_F16 && d->dtype != LA3D_DTYPE_U16) return refuse(who, "la3d_depth16: unknown dtype (LA3D_DTYPE_F16 or LA3D_DTYPE_U16)");
    if (d->dtype == LA3D_DTYPE_U16 ? (!(d->scale > 0.0f && d->scale <= 3.4028234663852886e38f) || (d->flags & ~LA3D_DEPTH_ZERO_IS_HOLE)) : d->flags != 0)
      return refuse(who, "la3d_depth16: U16 needs a finite scale > 0 and flags LA3D_DEPTH_ZERO_IS_HOLE or 0; F16 needs flags 0");
    if (!d->planes || (reinterpret_cast<uintptr_t>(d->planes) & 1)) return refuse(who, "la3d_depth16: planes NULL or not 2-byte aligned");
    if (a.depth_plane_stride != 0) return refuse(who, "depth_plane_stride must be 0 with depth16 (the block carries the stride)");
    if (d->dtype == LA3D_DTYPE_U16) { d16_scale = d->scale; d16_hole = (d->flags & LA3D_DEPTH_ZERO_IS_HOLE) ? 1 : 0; }
    dplanes = d->planes;
    dstride = d->plane_stride;
  } else if (reinterpret_cast<uintptr_t>(a.depth) & 3) return refuse(who, "depth not 4-byte aligned");
  if (dstride < 0 || a.mask_plane_stride < 0 || a.bits_plane_stride < 0) return refuse(who, "negative plane stride");
  if (a.k_stride != 0 && a.k_stride < 9) return refuse(who, "k_stride must be 0 (shared) or >= 9");
  if (!a.K) return refuse(who, "K is NULL");
  if (!a.workspace || (reinterpret_cast<uintptr_t>(a.workspace) & 3)) return refuse(who, "workspace NULL or not 4-byte aligned (la3d_instance_points_workspace_bytes)");
  if (!a.offsets) return refuse(who, "offsets is NULL");
  if (!gather && !a.counts) return refuse(who, "counts is NULL");
  // (capacity 0 - a batch of empty masks sized exactly - has no row to point at: points may be NULL there, no row is ever written)
  if (gather && ((!a.points && a.capacity > 0) || !a.status)) return refuse(who, "points / status is NULL");
  if (gather && a.capacity < 0) return refuse(who, "negative capacity");
  if (a.mask_bits && (reinterpret_cast<uintptr_t>(a.mask_bits) & 3)) return refuse(who, "mask_bits not 4-byte aligned");
  if (a.frames) {
    if (a.mask) return refuse(who, "a frames call takes bit planes (mask_bits + bits_offsets), not u8 masks");
    if (reinterpret_cast<uintptr_t>(a.frames) & 7) return refuse(who, "frames not 8-byte aligned");
    if (!a.bits_offsets || (reinterpret_cast<uintptr_t>(a.bits_offsets) & 7)) return refuse(who, "bits_offsets NULL or not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(a.mask_bits) & 15) return refuse(who, "mask_bits of a frames call not 16-byte aligned");
    if (!a.image_index) return refuse(who, "image_index is required: instance n belongs to frame row image_index[n]");
    if (dstride != 0 || a.frame_width != 0) return refuse(who, "depth plane stride and frame_width must be 0 in a frames call (the frame table says both)");
    if (reinterpret_cast<uintptr_t>(dplanes) & (a.depth16 ? 7 : 15)) return refuse(who, "the depth buffer of a frames call must be 16-byte (16-bit planes: 8-byte) aligned");
  } else {
    if (a.bits_offsets) return refuse(who, "bits_offsets without frames");
    const long long HW = (long long)a.H * a.W;
    if (a.mask && a.mask_plane_stride != 0 && a.mask_plane_stride < HW) return refuse(who, "mask_plane_stride below H*W");
    if (a.mask_bits && a.bits_plane_stride != 0 && a.bits_plane_stride < (HW + 31) / 32) return refuse(who, "bits_plane_stride below the words of a plane");
    if (dstride != 0 && dstride < HW) return refuse(who, "depth plane stride below H*W");
  }
  const int Wb = a.frames ? ((a.W + 31) & ~31) : a.W;   // (frames: W bounds the pitch)
  if (Wb > BAND_PIX) return refuse(who, "W > 65536: one row does not fit a band's bit image in LDS", LA3D_ERR_UNSUPPORTED);
  if ((long long)a.H * Wb > 0x7fffffffLL) return refuse(who, "H * W >= 2^31: pixel indices are int32", LA3D_ERR_UNSUPPORTED);
  const int nb = cloud_bands(a.B, a.H, Wb);
  if ((long long)a.B * nb > 0x7fffffffLL) return refuse(who, "B x bands >= 2^31: beyond one grid", LA3D_ERR_UNSUPPORTED);
  memset(&p, 0, sizeof(p));
  p.B = a.B; p.H = a.H; p.W = a.frames ? Wb : a.W; p.fw = a.frame_width ? a.frame_width : a.W; p.nb = nb; p.P = a.P;
  p.k_stride = a.k_stride; p.d16_hole = d16_hole; p.d16_scale = d16_scale;
  p.depth = dplanes; p.depth_stride = dstride;
  p.image_index = a.image_index;
  p.mask = a.mask; p.mask_stride = a.mask_plane_stride ? a.mask_plane_stride : (long long)a.H * a.W;
  p.bits = a.mask_bits; p.bits_stride = a.bits_plane_stride ? a.bits_plane_stride : ((long long)a.H * a.W + 31) / 32;
  p.bits_offsets = reinterpret_cast<const long long*>(a.bits_offsets);
  p.K = a.K; p.sample_idx = a.sample_idx; p.frames = a.frames;
  p.counts = a.counts; p.offsets = reinterpret_cast<long long*>(a.offsets); p.points = a.points; p.pixels = a.pixels; p.status = a.status; p.capacity = a.capacity;
  p.ws = static_cast<int*>(a.workspace);
  return LA3D_SUCCESS;
}

template <typename DT, bool FRAMES>
void launch_gather(const CloudParams& p, const DepthCvt<DT>& cv, bool f64, hipStream_t s) {
  const dim3 grid((unsigned)((long long)p.B * p.nb));
  if (f64) hipLaunchKernelGGL((cloud_gather_kernel<DT, double, FRAMES>), grid, dim3(CT), 0, s, p, cv);
  else hipLaunchKernelGGL((cloud_gather_kernel<DT, float, FRAMES>), grid, dim3(CT), 0, s, p, cv);
}

template <bool FRAMES>
void launch_gather_any(const CloudParams& p, int dtype, bool f64, hipStream_t s) {
  if (dtype == LA3D_DTYPE_F16) launch_gather<d_f16, FRAMES>(p, DepthCvt<d_f16>{}, f64, s);
  else if (dtype == LA3D_DTYPE_U16) {
    DepthCvt<d_u16> cv;
    cv.scale = p.d16_scale; cv.hole = p.d16_hole;
    launch_gather<d_u16, FRAMES>(p, cv, f64, s);
  } else launch_gather<float, FRAMES>(p, DepthCvt<float>{}, f64, s);
}
}  // namespace

extern "C" {

size_t la3d_instance_points_workspace_bytes(int B, int H, int W) {
  const int Wb = (W + 31) & ~31;   // (sized for the frames form too, whose pitches are multiples of 32)
  if (B <= 0 || H <= 0 || W <= 0 || Wb > BAND_PIX) return 0;
  const int nb_a = cloud_bands(B, H, W), nb_b = cloud_bands(B, H, Wb);
  return (size_t)B * (size_t)((nb_a > nb_b ? nb_a : nb_b) + 1) * sizeof(int32_t);
}

int la3d_instance_point_offsets(const la3d_cloud_args* args) {
  const char* who = "la3d_instance_point_offsets";
  la3d_cloud_args a;
  CloudParams p;
  const int rc = cloud_check(args, who, false, a, p);
  if (rc != LA3D_SUCCESS) return rc;
  hipStream_t s = static_cast<hipStream_t>(a.stream);
  if (a.B > 0) {
    const dim3 grid((unsigned)((long long)p.B * p.nb));
    if (a.frames) hipLaunchKernelGGL(cloud_count_kernel<true>, grid, dim3(CT), 0, s, p);
    else hipLaunchKernelGGL(cloud_count_kernel<false>, grid, dim3(CT), 0, s, p);
    const int rc2 = check_launch("cloud_count_kernel");
    if (rc2 != LA3D_SUCCESS) return rc2;
  }
  hipLaunchKernelGGL(cloud_scan_kernel, dim3(1), dim3(ST), 0, s, p);   // (B == 0: offsets[0] = 0)
  return check_launch("cloud_scan_kernel");
}

int la3d_gather_instance_points(const la3d_cloud_args* args) {
  const char* who = "la3d_gather_instance_points";
  la3d_cloud_args a;
  CloudParams p;
  const int rc = cloud_check(args, who, true, a, p);
  if (rc != LA3D_SUCCESS) return rc;
  if (a.B == 0) return LA3D_SUCCESS;
  hipStream_t s = static_cast<hipStream_t>(a.stream);
  const dim3 sgrid((unsigned)((a.B + CT / 64 - 1) / (CT / 64)));
  if (a.frames) hipLaunchKernelGGL(cloud_status_kernel<true>, sgrid, dim3(CT), 0, s, p);
  else hipLaunchKernelGGL(cloud_status_kernel<false>, sgrid, dim3(CT), 0, s, p);
  const int rc2 = check_launch("cloud_status_kernel");
  if (rc2 != LA3D_SUCCESS) return rc2;
  const int dtype = a.depth16 ? a.depth16->dtype : LA3D_DTYPE_F32;
  if (a.frames) launch_gather_any<true>(p, dtype, a.out_is_f64 != 0, s);
  else launch_gather_any<false>(p, dtype, a.out_is_f64 != 0, s);
  return check_launch("cloud_gather_kernel");
}

}  // extern "C"
