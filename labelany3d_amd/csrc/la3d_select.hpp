// la3d_select.hpp - the exact float32 median of the values under a bit image, for one 512-thread workgroup: what la3d_consumers.hip
// (la3d_masked_ratio_median: the ratio of two planes) and la3d_depth_gate.hip (la3d_depth_gate_bits: a depth plane, then its absolute
// deviations) share.  The caller holds the bit image of the pixels that count in LDS and the list of the 64-pixel chunks that hold one;
// masked_median gives np.median of their values:
//   fast     sample -> bracket -> one counting sweep -> one collecting sweep -> exact select in LDS: see the block marked "fast path";
//            falls through to the rounds below whenever a count does not confirm it
//   rounds   the k-th smallest value is found exactly by a most-significant-first radix select on an order-preserving key,
//            four rounds of 8 bits; a wave takes 64 consecutive pixels per step (coalesced 256-byte loads, chunks without a pixel
//            are skipped), so the values are re-derived from memory once per round instead of being kept.  Values of one mask
//            share their leading bits, so a plain LDS histogram would serialise on a handful of bins: every bin has 16 copies (one
//            per lane & 15, laid out [bin][copy] so that equal bins fall on different banks) - at most four lanes of a wave ever
//            meet on one word.
//   even n   np.median averages the two middle values (in float32).  The upper one equals the lower one when the lower
//            key occurs often enough; otherwise it is the smallest key above it (one more sweep with an LDS atomicMin).
// Any NaN value makes the result NaN, as np.median does.  Integer LDS atomics only: the result is a selection, so it depends neither
// on the order the atomics land in nor on the run.
// A VALUE (template argument V) says how a pixel's value is made: `In` is what is loaded per pixel, idle() what a lane without a pixel
// holds, load(i) the loads of pixel i - issued for several chunks before any is used -, value(x) the float32 that is ranked.
#pragma once
#include "la3d_device.hpp"

using namespace la3d;

namespace {
__device__ inline unsigned f32_key(float v) {
  const unsigned b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ inline float f32_unkey(unsigned k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

constexpr int RM_COPIES = 16;

constexpr int RM_NT = 512;   // threads per workgroup
constexpr int RM_CAP = 6144; // keys the LDS buffer of the fast path holds (sample, then the candidates of the median's bin)
// the LDS words masked_median works in behind the caller's bit image: the key buffer / histogram, the bracket's bins, the bin totals, misc
constexpr int RM_WORK_WORDS = RM_CAP + 1024 + 256 + 16;

// Keys at ranks ra <= rb (0-based, ascending) among the m keys in LDS buf: most-significant-first radix select, four rounds of
// 8 bits, both ranks at once (wave 0 follows ra, wave 1 follows rb).  h2: LDS [2][256]; st: LDS [4] = prefix a, rank a, prefix b,
// rank b (initialised here).  Every thread of the workgroup calls it; results in st[0], st[2] after the final barrier.
__device__ inline void lds_select2(const unsigned* buf, int m, unsigned ra, unsigned rb, unsigned* h2, unsigned* st, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { st[0] = 0u; st[1] = ra; st[2] = 0u; st[3] = rb; }
  unsigned pmask = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    h2[tid] = 0u;                        // RM_NT == 512 == 2 * 256
    __syncthreads();
    const unsigned pa = st[0], pb = st[2];
    for (int i = tid; i < m; i += RM_NT) {
      const unsigned k = buf[i], d = (k >> shift) & 0xffu;
      if ((k & pmask) == pa) atomicAdd(&h2[d], 1u);
      if ((k & pmask) == pb) atomicAdd(&h2[256 + d], 1u);
    }
    __syncthreads();
    if (wave < 2) {                      // four bins per lane, exclusive scan over the lanes
      const unsigned* h = h2 + 256 * wave;
      const unsigned b0 = h[4 * lane], b1 = h[4 * lane + 1], b2 = h[4 * lane + 2], b3 = h[4 * lane + 3];
      const unsigned mine = b0 + b1 + b2 + b3;
      unsigned incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
      }
      const unsigned rank = st[2 * wave + 1], excl = incl - mine;
      if (excl <= rank && rank < incl) { // exactly one lane
        unsigned acc = excl, bsel = 0;
        if (rank >= acc + b0) { acc += b0; bsel = 1;
          if (rank >= acc + b1) { acc += b1; bsel = 2;
            if (rank >= acc + b2) { acc += b2; bsel = 3; } } }
        st[2 * wave] = st[2 * wave] | ((4u * (unsigned)lane + bsel) << shift);
        st[2 * wave + 1] = rank - acc;
      }
    }
    pmask |= 0xffu << shift;
    __syncthreads();
  }
}

// the bit of the caller's bit image that belongs to this lane's pixel of chunk c (64 pixels = words 2c, 2c + 1)
__device__ inline unsigned chunk_bit(const unsigned* bits, int nwords, int c, int lane) {
  const unsigned w0 = bits[2 * c], w1 = (2 * c + 1 < nwords) ? bits[2 * c + 1] : 0u;
  return lane < 32 ? (w0 >> lane) & 1u : (w1 >> (lane - 32)) & 1u;
}

// The ids of the chunks (of nchunks) that hold a pixel of the bit image -> clist, in any order; their number is added to *nact (LDS,
// zero before the call).  Every thread of the workgroup calls it; no barrier: the caller's follows.
__device__ inline void list_active_chunks(const unsigned* bits, int nwords, int nchunks, unsigned short* clist, unsigned* nact, int tid) {
  const int lane = tid & 63;
  for (int c0 = 0; c0 < nchunks; c0 += RM_NT) {
    const int c = c0 + tid;
    const bool act = c < nchunks && ((bits[2 * c] | ((2 * c + 1 < nwords) ? bits[2 * c + 1] : 0u)) != 0);
    const unsigned long long bal = __ballot(act);
    unsigned base = 0;
    if (lane == 0 && bal) base = atomicAdd(nact, (unsigned)__popcll(bal));
    base = __shfl(base, 0);
    if (act) clist[base + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)c;
  }
}

// One sweep of the fast path over the chunks that hold a pixel (every cstep-th one).  MODE 0: append every key to buf
// (the sample).  MODE 1: count the keys below klo, histogram those in [klo, khi] by (key - klo) >> sh (256 bins x 4 copies),
// note NaN values.  MODE 2: append the keys in [klo, khi] to buf.  cnt: LDS counter of appended keys (entries beyond RM_CAP are
// dropped but counted); lt: LDS counter; nanflag: LDS.
template <int MODE, class V>
__device__ inline void rm_sweep(const V& val, const unsigned* bits, int nwords, const unsigned short* clist, int nact, int cstep,
                                unsigned klo, unsigned khi, int sh, unsigned* buf, unsigned* cnt, unsigned* h1, unsigned* lt,
                                unsigned* nanflag, int wave, int lane) {
  constexpr int U = 8;     // chunks in flight per wave
  unsigned lt_local = 0, nan_local = 0;
  for (int j0 = wave * U * cstep; j0 < nact; j0 += (RM_NT / 64) * U * cstep) {
    typename V::In x[U];
    unsigned on[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      on[u] = 0; x[u] = val.idle();
      const int j = j0 + u * cstep;
      if (j < nact) {
        const int c = clist[j];
        on[u] = chunk_bit(bits, nwords, c, lane);
        if (on[u]) x[u] = val.load(c * 64 + lane);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (j0 + u * cstep >= nact) continue;   // uniform
      const float r = val.value(x[u]);
      const unsigned key = f32_key(r);
      bool take = on[u] != 0;
      if (MODE == 1) {
        if (take) {
          nan_local |= (r != r) ? 1u : 0u;
          lt_local += key < klo ? 1u : 0u;
          if (key >= klo && key <= khi) atomicAdd(&h1[((key - klo) >> sh) * 4 + (lane & 3)], 1u);
        }
        continue;
      }
      if (MODE == 2) take = take && key >= klo && key <= khi;
      const unsigned long long bal = __ballot(take);
      if (bal == 0) continue;
      unsigned base = 0;
      if (lane == 0) base = atomicAdd(cnt, (unsigned)__popcll(bal));
      base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
      if (take) {
        const unsigned pos = base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        if (pos < (unsigned)RM_CAP) buf[pos] = key;
      }
    }
  }
  if (MODE == 1) {
    lt_local = (unsigned)wave_sum_i((int)lt_local);
    if (lane == 0 && lt_local) atomicAdd(lt, lt_local);
    if (__ballot(nan_local != 0) != 0 && lane == 0) *nanflag = 1u;
  }
}

// The body of masked_median: thread 0 leaves the median's bits in misc[0]; every return is workgroup-uniform.
// misc: [0] the result, [1] nan flag, [2] prefix, [3] rank, [4] count of the selected bin, [5] min key above, [6] the caller's,
//       [7] appended keys, [8] keys below the bracket, [9] fast-path verdict, [10..13] lds_select2 state, [14] lo2, [15] hi2
template <class V>
__device__ inline void masked_median_run(const V& val, const unsigned n, const unsigned* bits, int nwords, const unsigned short* clist,
                                         const int nact, unsigned* hist, unsigned* h1, unsigned* bsum, unsigned* misc, const int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const auto leave = [&](float v) { if (tid == 0) misc[0] = __float_as_uint(v); };
  // ---- fast path (round 3): sample -> bracket -> one counting sweep -> one collecting sweep -> exact select in LDS --------
  // The four radix rounds below visit every pixel four (five) times, each time re-deriving the value from its loads, and they are
  // latency-bound.  Here: (0) the keys of every cstep-th active chunk (~2-4 k keys) go to LDS and two
  // of their order statistics, 50 % -/+ 1/12, bracket the median; (1) one sweep counts the keys below the bracket and
  // histograms the keys inside it in <= 256 power-of-two bins; the bin(s) holding the middle rank(s) hold n / 1000 keys or so;
  // (2) one sweep collects exactly those keys; (3) an in-LDS radix select gives the exact middle value(s).  Every step is
  // verified by counts: if the bracket misses the median, a bin overflows the buffer, or the sample was too small, the
  // verdict stays 0 and the radix rounds below run as before.  A mask of <= RM_CAP pixels is selected from step (0) alone.
  {
    unsigned* st = misc + 10;
    const unsigned rlo = (n & 1u) ? n / 2 : n / 2 - 1, rhi = n / 2;       // 0-based ranks of the middle value(s)
    constexpr unsigned RM_SAMPLE = 2048u;   // keys the bracket is estimated from
    const int cstep = (int)(n <= (unsigned)RM_CAP ? 1u : (n + RM_SAMPLE - 1u) / RM_SAMPLE);
    rm_sweep<0>(val, bits, nwords, clist, nact, cstep, 0u, 0xffffffffu, 0, hist, &misc[7], h1, &misc[8], &misc[1], wave, lane);
    __syncthreads();
    const unsigned ns_all = misc[7];
    const int ns = (int)(ns_all < (unsigned)RM_CAP ? ns_all : (unsigned)RM_CAP);
    if (cstep == 1 && ns_all == n) {     // uniform: every key is in LDS - select directly (NaN keys sort last: check them here)
      unsigned nanl = 0;
      for (int i = tid; i < ns; i += RM_NT) nanl |= (hist[i] > 0xff800000u || (hist[i] < 0x007fffffu)) ? 1u : 0u;   // NaN keys
      if (__ballot(nanl != 0) != 0 && lane == 0) misc[1] = 1u;
      lds_select2(hist, ns, rlo, rhi, h1, st, tid);
      const float v0 = f32_unkey(st[0]), v1 = f32_unkey(st[2]);
      return leave(misc[1] ? NAN : ((n & 1u) ? v0 : (v0 + v1) / 2.0f));
    }
    if (ns >= 512) {                     // uniform: enough of a sample to bracket with
      const unsigned w = (unsigned)ns / 12u;
      lds_select2(hist, ns, (unsigned)ns / 2u - w, (unsigned)ns / 2u + w, h1, st, tid);
      const unsigned klo = st[0], khi = st[2];
      const unsigned width = khi - klo;
      const int sh = width < 256u ? 0 : (32 - __clz((int)width)) - 8;    // (width >> sh) < 256
      __syncthreads();                   // everyone has read st before the counters are reused
      for (int i = tid; i < 1024; i += RM_NT) h1[i] = 0u;
      if (tid == 0) { misc[7] = 0u; misc[8] = 0u; }
      __syncthreads();
      rm_sweep<1>(val, bits, nwords, clist, nact, 1, klo, khi, sh, hist, &misc[7], h1, &misc[8], &misc[1], wave, lane);
      __syncthreads();
      if (misc[1] != 0) return leave(NAN);   // uniform: a NaN value
      if (tid < 256) bsum[tid] = h1[4 * tid] + h1[4 * tid + 1] + h1[4 * tid + 2] + h1[4 * tid + 3];
      __syncthreads();
      if (tid == 0) {                    // (256 bins, one thread: ~1 us, once per median)
        const unsigned below = misc[8];
        unsigned acc = below, b0 = 256, b1 = 256, before = 0;
        for (unsigned b = 0; b < 256; ++b) {
          const unsigned c = bsum[b];
          if (b0 == 256 && rlo >= acc && rlo < acc + c) { b0 = b; before = acc; }
          if (b1 == 256 && rhi >= acc && rhi < acc + c) b1 = b;
          acc += c;
        }
        unsigned ok = (rlo >= below && b0 < 256 && b1 < 256) ? 1u : 0u;
        unsigned tot = 0;
        if (ok) {
          for (unsigned b = b0; b <= b1; ++b) tot += bsum[b];
          if (tot > (unsigned)RM_CAP) ok = 0;
        }
        misc[9] = ok;
        if (ok) {
          misc[14] = klo + (b0 << sh);
          const unsigned long long top = (unsigned long long)klo + ((unsigned long long)(b1 + 1) << sh) - 1ull;
          misc[15] = top > (unsigned long long)khi ? khi : (unsigned)top;
          misc[4] = rlo - before; misc[3] = rhi - before; misc[2] = tot;
        }
      }
      __syncthreads();
      if (misc[9] != 0) {                // uniform
        rm_sweep<2>(val, bits, nwords, clist, nact, 1, misc[14], misc[15], 0, hist, &misc[7], h1, &misc[8], &misc[1], wave, lane);
        __syncthreads();
        if (misc[7] == misc[2]) {        // uniform: exactly the keys the histogram promised
          lds_select2(hist, (int)misc[7], misc[4], misc[3], h1, st, tid);
          const float v0 = f32_unkey(st[0]), v1 = f32_unkey(st[2]);
          return leave((n & 1u) ? v0 : (v0 + v1) / 2.0f);
        }
      }
    }
    __syncthreads();
    if (tid < 16 && tid != 0 && tid != 6) misc[tid] = tid == 5 ? 0xffffffffu : 0u;   // back to the state the radix rounds expect
    if (tid == 0) misc[3] = (n & 1u) ? n / 2 : n / 2 - 1;
    __syncthreads();
  }
  const int copy = lane & (RM_COPIES - 1);
  unsigned pmask = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < 256 * RM_COPIES; i += RM_NT) hist[i] = 0;
    __syncthreads();                     // also publishes misc[2..3] of the previous round
    const unsigned prefix = misc[2];
    unsigned nan_local = 0;
    constexpr int RM_U = 4;      // chunks in flight per wave: the loads of RM_U chunks are issued before any is used
    for (int j0 = wave * RM_U; j0 < nact; j0 += (RM_NT / 64) * RM_U) {
      typename V::In x[RM_U];
      unsigned on[RM_U];
#pragma unroll
      for (int u = 0; u < RM_U; ++u) {
        on[u] = 0; x[u] = val.idle();
        if (j0 + u < nact) {
          const int c = clist[j0 + u];
          on[u] = chunk_bit(bits, nwords, c, lane);
          if (on[u]) x[u] = val.load(c * 64 + lane);
        }
      }
#pragma unroll
      for (int u = 0; u < RM_U; ++u) {
        if (on[u]) {
          const float r = val.value(x[u]);
          if (shift == 24) nan_local |= (r != r) ? 1u : 0u;
          const unsigned key = f32_key(r);
          if ((key & pmask) == prefix) atomicAdd(&hist[((key >> shift) & 0xffu) * RM_COPIES + copy], 1u);
        }
      }
    }
    if (shift == 24 && __ballot(nan_local != 0) != 0 && lane == 0) misc[1] = 1u;
    __syncthreads();
    if (shift == 24 && misc[1] != 0) return leave(NAN);   // uniform
    if (tid < 256) {   // bin totals, then the bin holding the wanted rank (wave 0: four bins per lane, exclusive scan over the lanes)
      unsigned t = 0;
#pragma unroll
      for (int k = 0; k < RM_COPIES; ++k) t += hist[tid * RM_COPIES + k];
      bsum[tid] = t;
    }
    __syncthreads();
    if (wave == 0) {
      const unsigned b0 = bsum[4 * lane], b1 = bsum[4 * lane + 1], b2 = bsum[4 * lane + 2], b3 = bsum[4 * lane + 3];
      const unsigned mine = b0 + b1 + b2 + b3;
      unsigned incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
      }
      const unsigned rank = misc[3], excl = incl - mine;
      if (excl <= rank && rank < incl) {   // exactly one lane
        unsigned acc = excl, bsel = 0, cnt = b0;
        if (rank >= acc + b0) { acc += b0; bsel = 1; cnt = b1;
          if (rank >= acc + b1) { acc += b1; bsel = 2; cnt = b2;
            if (rank >= acc + b2) { acc += b2; bsel = 3; cnt = b3; } } }
        misc[2] = prefix | ((4u * (unsigned)lane + bsel) << shift);
        misc[3] = rank - acc;
        misc[4] = cnt;
      }
    }
    pmask |= 0xffu << shift;
    __syncthreads();
  }
  const unsigned key0 = misc[2];
  unsigned key1 = key0;
  if (!(n & 1u) && misc[3] + 1 >= misc[4]) {   // uniform: the upper middle value is the smallest key above key0
    for (int j = wave; j < nact; j += RM_NT / 64) {
      const int c = clist[j];
      unsigned k = 0xffffffffu;
      if (chunk_bit(bits, nwords, c, lane)) {
        const unsigned key = f32_key(val.value(val.load(c * 64 + lane)));
        if (key > key0) k = key;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) k = min(k, (unsigned)__shfl_xor((int)k, o));
      if (lane == 0 && k != 0xffffffffu) atomicMin(&misc[5], k);
    }
    __syncthreads();
    key1 = misc[5];
  }
  const float v0 = f32_unkey(key0);
  leave((n & 1u) ? v0 : (v0 + f32_unkey(key1)) / 2.0f);   // float32 mean of the two middle values
}

// np.median (float32) of the n > 0 values under the bit image `bits` (nwords words in LDS), to every thread of the workgroup.  clist:
// the ids of the nact 64-pixel chunks that hold a pixel, in any order.  hist (RM_CAP words), h1 (1024), bsum (256), misc (16): LDS the
// call works in; misc[6] alone is left as it is.  Every thread of the workgroup calls it, with the same arguments; it may be called
// again at once (each call begins with a barrier and sets up its own state).
template <class V>
__device__ inline float masked_median(const V& val, unsigned n, const unsigned* bits, int nwords, const unsigned short* clist, int nact,
                                      unsigned* hist, unsigned* h1, unsigned* bsum, unsigned* misc, int tid) {
  __syncthreads();                       // whatever read misc, hist or the chunk list's counter before is done
  if (tid < 16 && tid != 6) misc[tid] = tid == 5 ? 0xffffffffu : tid == 3 ? ((n & 1u) ? n / 2 : n / 2 - 1) : 0u;   // [3]: 0-based rank of the (lower) middle value
  __syncthreads();
  masked_median_run(val, n, bits, nwords, clist, nact, hist, h1, bsum, misc, tid);
  __syncthreads();
  return __uint_as_float(misc[0]);
}
}  // namespace
