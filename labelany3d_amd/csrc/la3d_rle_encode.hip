// la3d_rle_encode.hip - the way back out of a bit plane (include/la3d.h "bit planes as run lengths"): the run-length encoder,
// la3d_rle_encode_offsets / la3d_rle_encode.  The planes are the SOURCE of the call: a BitsOut that is only read, checked by pack_check
// (la3d_bitplanes.hpp) in either form.
#include <cstdint>
#include <cstddef>
#include <cstring>

#include "la3d_bitplanes.hpp"

namespace {
// ---- bit planes -> COCO run lengths (la3d_rle_encode_offsets / la3d_rle_encode) --------------------------------------------------
// binary_mask_to_rle for a batch (reference src/download_coconut.py:167-175): the runs of the (H, frame_width) image in COLUMN-major
// order (flat = u * H + v), zeros first.  A transition is a flat index i > 0 whose pixel differs from pixel i - 1; with T transitions
// at p_1 < ... < p_T, p_0 = 0 and p_{T+1} = H * frame_width the run list is [p_1 - p_0, ..., p_{T+1} - p_T], led by a 0 when pixel
// (0, 0) is set: T + 1 + bit(0, 0) counts.
// One workgroup per instance streams the plane into LDS (bits_plane_to_lds: the consumers' copy) and gives every image column a thread
// that walks it top to bottom - the 64 lanes of a wave read the same one or two LDS words of a row (a broadcast), each its own bit.
// Only bits (v, u) with v < H and u < frame_width are looked at: pad columns and the spare bits of the last word are never mask.
//   stage 1  per column: T[u], its transitions, and L[u], the row of its last one (-1: none) -> workspace; runs[n] = sum T + 1 + bit(0, 0)
//   stage 2  T and L come back from the workspace; a scan over the columns (a sum for the rank, a maximum for the position of the
//            transition before the column: shuffles inside a wave, the wave totals through LDS, a carry from chunk to chunk of NT_DEC
//            columns) tells every thread the index of its first count and the position that count starts from, so the second walk
//            stores each count where it belongs: no atomics, no ordering between threads.  Every store is guarded by the instance's
//            own range, so a plane that changed after stage 1 (or a foreign workspace) can only spoil values inside that range.
struct RleOut {
  int* runs;                  // [B], stage 1
  long long* offsets;         // [B + 1]: written by stage 1, read by stage 2
  int* counts;                // [capacity], stage 2
  int* status;                // [B], stage 2
  long long capacity;
  int2* ws;                   // [B][ws_cols]: (T, L) of every column
  int ws_cols;
};
constexpr size_t RLE_SCAN_BYTES = 2 * (NT_DEC / 64) * sizeof(int);   // behind the bit image (16-aligned): the wave totals of the scan

// bit (v, u) of an LDS bit image whose rows lie W bits apart, for v = 0 .. H - 1: on(v) is called wherever it differs from the pixel
// before it in column-major order - (v - 1, u), or (H - 1, u - 1) for v = 0; pixel (0, 0) has none
template <typename F>
__device__ inline void column_transitions(const unsigned* bits, int H, int W, int u, F&& on) {
  const int before = u > 0 ? (H - 1) * W + u - 1 : 0;
  unsigned prev = (bits[before >> 5] >> (before & 31)) & 1u;
  if ((W & 31) == 0) {   // uniform: rows of whole words - one word index per row, one shift for the column
    // eight rows per step: eight independent LDS reads, their bits gathered into m, the transitions among them as the set bits of
    // x = m ^ (m shifted by one row) - most steps of a real mask have none, and the loop over them is skipped
    const unsigned* p = bits + (u >> 5);
    const int wpr = W >> 5, sh = u & 31;
    int v = 0;
    for (; v + 8 <= H; v += 8) {
      unsigned m = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) m |= ((p[(v + k) * wpr] >> sh) & 1u) << k;
      unsigned x = (m ^ ((m << 1) | prev)) & 0xffu;
      prev = m >> 7;
      while (x) {
        on(v + __ffs((int)x) - 1);
        x &= x - 1u;
      }
    }
    for (; v < H; ++v) {
      const unsigned b = (p[v * wpr] >> sh) & 1u;
      if (b != prev) on(v);
      prev = b;
    }
  } else {
    int i = u;
    for (int v = 0; v < H; ++v, i += W) {
      const unsigned b = (bits[i >> 5] >> (i & 31)) & 1u;
      if (b != prev) on(v);
      prev = b;
    }
  }
}

// Over the NTH threads of the workgroup: the exclusive prefix of a sum (t) and of a maximum (p >= 0), and both totals.  Every thread
// calls it; sc: LDS, 2 * NTH / 64 ints, free again when it returns.
template <int NTH>
__device__ inline void block_scan_sum_max(int t, int p, int* sc, int tid, int* ex_t, int* ex_p, int* tot_t, int* tot_p) {
  const int lane = tid & 63, wave = tid >> 6;
  int it = t, ip = p;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int a = __shfl_up(it, d), b = __shfl_up(ip, d);
    if (lane >= d) { it += a; ip = max(ip, b); }
  }
  const int before_p = __shfl_up(ip, 1);
  if (lane == 63) { sc[wave] = it; sc[NTH / 64 + wave] = ip; }
  __syncthreads();
  int bt = 0, bp = 0, st = 0, sp = 0;
#pragma unroll
  for (int w = 0; w < NTH / 64; ++w) {
    const int a = sc[w], b = sc[NTH / 64 + w];
    if (w < wave) { bt += a; bp = max(bp, b); }
    st += a; sp = max(sp, b);
  }
  __syncthreads();
  *ex_t = bt + it - t;
  *ex_p = lane > 0 ? max(bp, before_p) : bp;
  *tot_t = st; *tot_p = sp;
}

template <bool FRAMES>
__global__ __launch_bounds__(NT_DEC) void rle_encode_count_kernel(const BitsOut c, const RleOut e) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, n = blockIdx.x;
  PlaneGeo g;
  if (!plane_geometry<FRAMES>(c, n, &g)) {   // (uniform) refused: nothing is read, no run
    if (tid == 0) e.runs[n] = 0;
    return;
  }
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  int* sc = reinterpret_cast<int*>(smem + (((size_t)c.lds_words * 4 + 15) & ~(size_t)15));
  (void)bits_plane_to_lds<NT_DEC>(g.out, bits, g.nwords, g.H * g.W, g.vec, tid);
  __syncthreads();
  const int fw = g.fw > 0 ? g.fw : g.W;   // the image columns
  int2* ws = e.ws + (long long)n * e.ws_cols;
  int total = 0;
  for (int u = tid; u < fw; u += NT_DEC) {
    int T = 0, L = -1;
    column_transitions(bits, g.H, g.W, u, [&](int v) { ++T; L = v; });
    ws[u] = make_int2(T, L);
    total += T;
  }
  total = wave_sum_i(total);
  if ((tid & 63) == 0) sc[tid >> 6] = total;
  __syncthreads();
  if (tid == 0) {
    int s = 1 + (int)(bits[0] & 1u);
#pragma unroll
    for (int w = 0; w < NT_DEC / 64; ++w) s += sc[w];
    e.runs[n] = s;
  }
}

// One workgroup: offsets = the exclusive prefix of runs.  Thread t owns a run of consecutive instances, the runs are scanned in LDS:
// deterministic, any B (the scan of la3d_instance_point_offsets).  B == 0: offsets[0] = 0.
constexpr int RLE_ST = 1024;
__global__ __launch_bounds__(RLE_ST) void rle_encode_scan_kernel(const int* __restrict__ runs, long long* __restrict__ offsets, int B) {
  __shared__ long long part[RLE_ST];
  const int tid = threadIdx.x;
  const int chunk = (B + RLE_ST - 1) / RLE_ST;
  const int n0 = (int)min((long long)B, (long long)tid * chunk), n1 = (int)min((long long)B, (long long)n0 + chunk);
  long long sum = 0;
  for (int n = n0; n < n1; ++n) sum += runs[n];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < RLE_ST; d <<= 1) {
    const long long t = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += t;
    __syncthreads();
  }
  long long run = part[tid] - sum;
  if (tid == 0) offsets[0] = 0;
  for (int n = n0; n < n1; ++n) {
    run += runs[n];
    offsets[n + 1] = run;
  }
}

template <bool FRAMES>
__global__ __launch_bounds__(NT_DEC) void rle_encode_emit_kernel(const BitsOut c, const RleOut e) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, n = blockIdx.x;
  PlaneGeo g;
  if (!plane_geometry<FRAMES>(c, n, &g)) {   // (uniform) refused: nothing is read or written
    if (tid == 0) e.status[n] = LA3D_BOX_UNSUPPORTED;
    return;
  }
  const long long off0 = uniform_i64(e.offsets[n]), off1 = uniform_i64(e.offsets[n + 1]);
  if (off0 < 0 || off1 < off0 || off1 > e.capacity) {   // (uniform) no room: nothing of the instance is written
    if (tid == 0) e.status[n] = LA3D_RLE_NO_ROOM;
    return;
  }
  const long long len = off1 - off0;   // every store below goes to out[i] with 0 <= i < len
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  int* sc = reinterpret_cast<int*>(smem + (((size_t)c.lds_words * 4 + 15) & ~(size_t)15));
  (void)bits_plane_to_lds<NT_DEC>(g.out, bits, g.nwords, g.H * g.W, g.vec, tid);
  __syncthreads();
  const int H = g.H, fw = g.fw > 0 ? g.fw : g.W;
  const int lead = (int)(bits[0] & 1u);
  const int2* ws = e.ws + (long long)n * e.ws_cols;
  int* out = e.counts + off0;
  int carry_t = 0, carry_p = 0, bad = 0;
  for (int u0 = 0; u0 < fw; u0 += NT_DEC) {   // uniform trip count: every thread takes part in the scan
    const int u = u0 + tid;
    int wT = 0, wL = -1;
    if (u < fw) {
      const int2 w = ws[u];
      wT = w.x; wL = w.y;
    }
    if (wT < 0 || wT > H || wL < -1 || wL >= H || (wT == 0) != (wL < 0)) {   // not what stage 1 writes: nothing is derived from it
      bad = 1; wT = 0; wL = -1;
    }
    int ex_t, ex_p, tot_t, tot_p;
    block_scan_sum_max<NT_DEC>(wT, wL >= 0 ? u * H + wL : 0, sc, tid, &ex_t, &ex_p, &tot_t, &tot_p);
    if (u < fw) {
      int rank = lead + carry_t + ex_t;   // the count this column's first transition ends
      int prev = max(carry_p, ex_p);      // where that count starts: the transition before the column, or 0
      int T = 0, L = -1;
      column_transitions(bits, H, g.W, u, [&](int v) {
        const int p = u * H + v;
        if ((long long)rank < len) out[rank] = p - prev;
        prev = p; ++rank; ++T; L = v;
      });
      bad |= (T != wT || L != wL) ? 1 : 0;
    }
    carry_t += tot_t; carry_p = max(carry_p, tot_p);
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    const long long last = (long long)lead + carry_t;   // the count that ends at H * frame_width
    if (lead && len > 0) out[0] = 0;
    if (last < len) out[last] = H * fw - carry_p;
    e.status[n] = (bad || last + 1 != len) ? LA3D_RLE_MISMATCH : LA3D_RLE_OK;
  }
}

// ---- bit planes -> run lengths: the check of both stages, made before any launch.  The rules of the block itself come first; the
// planes then go through pack_check as the SOURCE of the call (a BitsOut that is only read), in either form.  RLE_NOTHING: B == 0.
enum { RLE_LAUNCH = 0, RLE_NOTHING = 1 };
int rle_encode_check(const la3d_rle_encode_args* args, const char* who, bool emit, la3d_rle_encode_args& a, BitsOut& c, RleOut& e) {
  static_assert(sizeof(la3d_rle_encode_args) == 120, "la3d_rle_encode_args is part of the ABI");
  if (!args || args->struct_size < (int32_t)sizeof(la3d_rle_encode_args)) return refuse(who, "bad struct_size");
  memcpy(&a, args, sizeof(a));   // (a longer block from a newer caller is fine)
  if (a.B < 0 || a.H < 0 || a.W < 0 || a.P < 0) return refuse(who, "negative sizes (B, H, W, P)");
  if (a.frame_width < 0 || a.frame_width > a.W) return refuse(who, "frame_width outside [0, W]");
  if (a.bits_plane_stride < 0) return refuse(who, "negative bits_plane_stride");
  if (emit && a.capacity < 0) return refuse(who, "negative capacity");
  if (a.bits_offsets && !a.frames) return refuse(who, "bits_offsets without frames");
  if (a.frames && !a.image_index) return refuse(who, "frames without image_index: instance n belongs to frame row image_index[n]");
  if (a.frames && (a.frame_width != 0 || a.bits_plane_stride != 0))
    return refuse(who, "frame_width and bits_plane_stride must be 0 in a frames call (the frame table and bits_offsets say both)");
  if (!a.offsets || (reinterpret_cast<uintptr_t>(a.offsets) & 7)) return refuse(who, "offsets NULL or not an 8-byte aligned pointer");
  memset(&e, 0, sizeof(e));
  e.runs = a.runs; e.offsets = reinterpret_cast<long long*>(a.offsets); e.counts = a.counts; e.status = a.status; e.capacity = a.capacity;
  e.ws = static_cast<int2*>(a.workspace); e.ws_cols = a.W;
  if (a.B == 0) return RLE_NOTHING;
  static const char* const p8 = "frames, bits_offsets or workspace not an 8-byte aligned pointer";
  static const char* const p4 = "image_index, runs, counts or status not a 4-byte aligned pointer";
  static const char* const nul = "NULL mask_bits, bits_offsets, runs, counts, status or workspace";
  uint32_t* planes = const_cast<uint32_t*>(a.mask_bits);   // (read only: the kernels of this pair load through BitsOut::bits)
  const bool no_counts = a.capacity == 0;                   // (no count can be written: counts may be NULL)
  int rc;
  if (a.frames) {
    static const PackWords say = {"empty bounds (H, W > 0 with B > 0)", nullptr, nul, "the bit image of the bounds must fit LDS (H * roundup32(W) <= 1048576)",
                                  nullptr, nullptr};
    c = bits_out_frames(a.frames, a.P, a.H, a.W, a.image_index, planes, a.bits_offsets, nullptr);
    rc = pack_check(who, say, a.B, a.P, a.W, true, false, bounds_words(a.H, a.W) > (1LL << 15),
                    {{planes, 15, "mask_bits of a frames call not a 16-byte aligned pointer"}, {a.frames, 7, p8}, {a.bits_offsets, 7, p8},
                     {a.workspace, 7, p8}, {a.image_index, 3, p4}, {a.runs, 3, p4, emit}, {a.counts, 3, p4, !emit || no_counts},
                     {a.status, 3, p4, !emit}}, 0, c);
  } else {
    static const PackWords say = {"empty frame (H, W > 0 with B > 0)", nullptr, nul, "the bit image must fit LDS (H*W <= 1048576)", nullptr,
                                  "bits_plane_stride is smaller than la3d_mask_bits_words(H, W)"};
    const int fw = a.frame_width ? a.frame_width : a.W;
    const long long stride = a.bits_plane_stride ? (long long)a.bits_plane_stride : (long long)la3d_mask_bits_words(a.H, a.W);
    c = bits_out_uniform(a.H, fw, a.W, planes, stride, nullptr);
    rc = pack_check(who, say, a.B, 1, fw, true, false, plane_items(a.H, a.W) > (1LL << 20),
                    {{planes, 3, "mask_bits not a 4-byte aligned pointer"}, {a.workspace, 7, p8}, {a.runs, 3, p4, emit},
                     {a.counts, 3, p4, !emit || no_counts}, {a.status, 3, p4, !emit}}, 0, c);
  }
  return rc == PACK_LAUNCH ? RLE_LAUNCH : rc;   // (work is always true here: PACK_NOTHING does not come back)
}
inline size_t rle_encode_lds(const BitsOut& c) { return (((size_t)c.lds_words * 4 + 15) & ~(size_t)15) + RLE_SCAN_BYTES; }
}  // namespace

extern "C" {

size_t la3d_rle_encode_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * (size_t)W * sizeof(int2);   // (T, L) of every column of every instance
}

int la3d_rle_encode_offsets(const la3d_rle_encode_args* args) {
  const char* who = "la3d_rle_encode_offsets";
  la3d_rle_encode_args a;
  BitsOut c;
  RleOut e;
  const int rc = rle_encode_check(args, who, false, a, c, e);
  if (rc < 0) return rc;
  hipStream_t s = static_cast<hipStream_t>(a.stream);
  if (rc == RLE_LAUNCH) {
    if (a.frames) {
      allow_big_lds(reinterpret_cast<const void*>(rle_encode_count_kernel<true>));
      hipLaunchKernelGGL(rle_encode_count_kernel<true>, dim3((unsigned)a.B), dim3(NT_DEC), rle_encode_lds(c), s, c, e);
    } else {
      allow_big_lds(reinterpret_cast<const void*>(rle_encode_count_kernel<false>));
      hipLaunchKernelGGL(rle_encode_count_kernel<false>, dim3((unsigned)a.B), dim3(NT_DEC), rle_encode_lds(c), s, c, e);
    }
    const int rc2 = check_launch("rle_encode_count_kernel");
    if (rc2 != LA3D_SUCCESS) return rc2;
  }
  hipLaunchKernelGGL(rle_encode_scan_kernel, dim3(1), dim3(RLE_ST), 0, s, e.runs, e.offsets, a.B);   // (B == 0: offsets[0] = 0)
  return check_launch("rle_encode_scan_kernel");
}

int la3d_rle_encode(const la3d_rle_encode_args* args) {
  const char* who = "la3d_rle_encode";
  la3d_rle_encode_args a;
  BitsOut c;
  RleOut e;
  const int rc = rle_encode_check(args, who, true, a, c, e);
  if (rc != RLE_LAUNCH) return pack_done(rc);
  hipStream_t s = static_cast<hipStream_t>(a.stream);
  if (a.frames) {
    allow_big_lds(reinterpret_cast<const void*>(rle_encode_emit_kernel<true>));
    hipLaunchKernelGGL(rle_encode_emit_kernel<true>, dim3((unsigned)a.B), dim3(NT_DEC), rle_encode_lds(c), s, c, e);
  } else {
    allow_big_lds(reinterpret_cast<const void*>(rle_encode_emit_kernel<false>));
    hipLaunchKernelGGL(rle_encode_emit_kernel<false>, dim3((unsigned)a.B), dim3(NT_DEC), rle_encode_lds(c), s, c, e);
  }
  return check_launch("rle_encode_emit_kernel");
}

}  // extern "C"
