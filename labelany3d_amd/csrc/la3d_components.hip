// la3d_components.hip - connected components on bit planes (include/la3d.h "connected components on bit planes"):
// la3d_components_bits and its frames form, la3d_components_bits_frames: kernels and C entries in one unit.  From la3d_bitplanes.hpp
// come the planes of a frames call and their locator (FramesPlanes, frames_source, frames_dest), the realigned word of an image row
// (plane_row_word), the in-place rule (planes_overlap), at() and the wording shared with the packers.
#include <cstdint>
#include <cstddef>

#include "la3d_bitplanes.hpp"

namespace {
// ---- connected components on bit planes -----------------------------------------------------------------------------------------
// scipy.ndimage.label of a plane, then a choice among its components by area.  The plane is never expanded to a label per pixel: the
// unit of work is the RUN, a maximal horizontal span of set pixels within one image row.  One workgroup per plane; its segment of the
// workspace holds, per run in raster order, px = v * fw + x0, x1, and two more words (below); and rs[v], the index of row v's first run.
//   1  count    items = (row, aligned 32-column word), row-major; wave w owns a contiguous range of them and takes it 64 items at a
//               time, lane by lane (coalesced).  The rising edges of a word, w & ~((w << 1) | carry), are the runs that begin in
//               it; ONE exclusive scan over the workgroup gives every wave the runs before its range - raster order, nothing
//               depends on arrival.  More runs than max_runs: the plane is refused here (statistics -1, runs; zero plane), before
//               anything is indexed by a run.
//   2  list     the same walk again, a wave scan per step placing each item's runs: a rising edge writes px, a falling edge x1.  The
//               ends before an item are its starts before it, less one when a run crosses into it, so neither looks for the other.
//   3  join     thread per run: the runs of the row above that overlap it (8: touching by one column counts; 4: a shared column) by a
//               binary search over that row, each joined by the lock-free union: the LARGER root is linked below the smaller with an
//               integer atomic min, so the partition and every root - the first run of its component in raster order - are the same
//               whatever the waves' order.
//   4  flatten  parent[i] = root; area[root] += length (integer atomic add).
//   5  choose   the roots in index order ARE the labels in SciPy's order: the rank of a root is a scan over threads that each own a
//               contiguous range of runs.  largest: the greatest area among the candidates, then the lowest root with it.  The area
//               word of a root becomes its tag: label | kept << 31.
//   6  write    table rectangles (integer atomic min / max into the caller's table rows, finished by a last pass), the rectangle of
//               the output, and the output words: thread per word, gathered from the kept runs of the rows that cross it - every word
//               of the plane has one writer.
// parent lives in LDS (4 * max_runs bytes, dynamic) up to 32768 runs, else in the workspace (one code text, COMP_LDS); the other
// arrays are read and written with plain loads and stores between workgroup barriers.  A workgroup is 16 waves (the passes wait on
// dependent loads: the waves hide one another's) of 106 VGPRs - 4 waves per SIMD -, so a CU holds ONE workgroup whatever max_runs is;
// its LDS (4 * max_runs bytes: 64 KiB at the default 16384, 128 KiB at 32768, none beyond) never is what limits it.  Measured
// (profiles/components/RESULTS.md): two workgroups of 8 waves and 57 VGPRs per CU were slower at every batch size.
// FRAMES (la3d_components_bits_frames, images of different sizes): the same passes on a geometry formed per workgroup from the la3d_frame
// row of its plane (comp_plane, all of it wave-uniform: SGPRs).  H, W of the call are then the bounds of the table: they size the
// segment of the workspace (rs has the bound's rows), a plane uses its own rows of it.  A row the device refuses gets -2 in its
// statistics, zero table rows, and neither reads nor writes a plane word.
constexpr int COMP_NT = 1024;
constexpr int COMP_NW = COMP_NT / 64;
constexpr int COMP_LDS_RUNS = 32768;      // parent in LDS up to here
constexpr int COMP_MAX_RUNS = 524288;     // a plane of 2^20 pixels has no more

struct CompArgs {
  const unsigned* bits; long long stride;
  unsigned* out; long long out_stride;
  int H, W, fw, nw;                        // rows, pitch, image columns, aligned words per image row (frames form: H, W are the bounds)
  int nwords;                              // words of a plane
  int conn8, min_area, largest, max_runs, maxc;
  int* stats; int* comps;
  int* ws; long long ws_stride;            // ints per plane: 4 * max_runs + 2 * H
};
// frames form: a FramesPlanes (la3d_bitplanes.hpp) beside a CompArgs whose fields that speak of ONE plane (stride, out_stride, fw, nw,
// nwords) are unused - those are formed per workgroup (comp_plane).  A kernel argument of its own: the uniform instantiation never
// reads it, and its CompArgs is the block it always had.
// what a workgroup works on: the geometry of its plane, where it is read and where the result goes (NULL: statistics only)
struct CompPlane { int H, W, fw, nw, nwords; const unsigned* plane; unsigned* op; };

// The plane of workgroup b.  Uniform form: the argument block's own geometry, planes a stride apart.  Frames form: formed here from the
// la3d_frame row of image_index[b] by the locator of la3d_bitplanes.hpp (frames_source, then frames_dest where a plane is stored) -
// every value wave-uniform, checked before an address is formed from it.  The output has the input's geometry.  false: refused -
// nothing is read, nothing is written through it.
template <bool FRAMES>
__device__ inline bool comp_plane(const CompArgs& a, const FramesPlanes& fr, int b, CompPlane* g) {
  if constexpr (FRAMES) {
    FramesWork f;
    if (!frames_source(fr, a.bits, a.H, a.W, b, &f)) return false;
    long long oo = 0;
    if (a.out && !frames_dest(fr, b, f.nwords, &oo)) return false;
    g->H = f.r.H; g->W = f.r.W; g->fw = f.r.fw; g->nw = (f.r.fw + 31) >> 5; g->nwords = f.nwords;
    g->plane = a.bits + f.off;               // (formed only now: after the last check)
    g->op = a.out ? a.out + oo : nullptr;
  } else {
    g->H = a.H; g->W = a.W; g->fw = a.fw; g->nw = a.nw; g->nwords = a.nwords;
    g->plane = a.bits + (long long)b * a.stride;
    g->op = a.out ? a.out + (long long)b * a.out_stride : nullptr;
  }
  return true;
}

// word wc of image row v, aligned to the row's first column; columns at and beyond fw are zero whatever the plane holds
__device__ inline unsigned comp_row_word(const CompPlane& a, const unsigned* __restrict__ plane, int v, int wc) {
  return plane_row_word(plane, a.nwords, a.W, v, wc * 32, a.fw - wc * 32);
}

// item `it` = (row v, word wc): its word, carry = the pixel left of the word, next = the pixel right of it (both 0 outside the row's
// image columns).  Neighbouring lanes take neighbouring items: the loads of a wave fall into a few lines.
struct CompItem { int v, wc; unsigned x, carry, next; };
__device__ inline CompItem comp_item(const CompPlane& a, const unsigned* __restrict__ plane, int it) {
  CompItem i;
  i.v = it / a.nw; i.wc = it - i.v * a.nw;
  i.x = comp_row_word(a, plane, i.v, i.wc);
  i.carry = i.wc ? comp_row_word(a, plane, i.v, i.wc - 1) >> 31 : 0u;
  i.next = i.wc + 1 < a.nw ? comp_row_word(a, plane, i.v, i.wc + 1) & 1u : 0u;
  return i;
}
__device__ inline int comp_wave_scan(int v) {   // inclusive, over the 64 lanes of a wave (all of them active)
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// exclusive scan of one int per thread over the workgroup; *total = the sum.  red: COMP_NW + 1 ints of LDS.  Ends with a barrier.
__device__ inline int comp_scan(int v, int* red, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = comp_wave_scan(v);
  __syncthreads();                         // (red may still be read from the call before)
  if (lane == 63) red[wave] = incl;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < COMP_NW; ++w) { const int r = red[w]; if (w < wave) base += r; sum += r; }
  *total = sum;
  return base + incl - v;
}
enum { COMP_SUM, COMP_MIN, COMP_MAX };
template <int OP>
__device__ inline int comp_reduce(int v, int* red) {
  v = OP == COMP_SUM ? wave_sum_i(v) : OP == COMP_MIN ? wave_min_i(v) : wave_max_i(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
#pragma unroll
  for (int w = 1; w < COMP_NW; ++w) r = OP == COMP_SUM ? r + red[w] : OP == COMP_MIN ? min(r, red[w]) : max(r, red[w]);
  return r;
}

// parent is read and linked while other waves link: relaxed atomics, so that no value is kept in a register across a retry.  Every
// value ever stored in parent[x] is a run of x's component with an index <= x, and a slot only decreases: whatever a find reads, it
// walks down inside the component and ends at a run that was a root when it was read.
__device__ inline int comp_ld(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline int comp_find(int* parent, int x) {
  const int x0 = x;
  int p = comp_ld(parent + x);
  while (p != x) { x = p; p = comp_ld(parent + x); }
  if (x < x0) atomicMin(parent + x0, x);   // one step of compression: the next find from x0 starts at the root it found
  return x;
}
__device__ inline void comp_unite(int* parent, int a, int b) {
  for (;;) {
    a = comp_find(parent, a); b = comp_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }        // a > b: the larger root goes below the smaller
    const int old = atomicMin(parent + a, b);
    if (old == a) return;                                 // a was a root and now points to b
    a = old;                                              // another wave linked a meanwhile: what it pointed to joins b as well
  }
}

template <bool COMP_LDS, bool FRAMES>
__global__ __launch_bounds__(COMP_NT) void components_kernel(const CompArgs a, const FramesPlanes fr) {
  extern __shared__ __attribute__((aligned(16))) int comp_smem[];
  __shared__ int red[COMP_NW + 1];
  const int tid = threadIdx.x, b = blockIdx.x;
  CompPlane g;
  const bool conforming = comp_plane<FRAMES>(a, fr, b, &g);
  int* stats = a.stats ? a.stats + (long long)b * 8 : nullptr;
  int* table = a.comps ? a.comps + (long long)b * a.maxc * 5 : nullptr;
  if (!conforming) {                       // (uniform, before any barrier) refused: the rows addressed by b alone say so
    if (stats && tid < 8) stats[tid] = tid == 0 ? -2 : 0;
    if (table) for (int j = tid; j < a.maxc * 5; j += COMP_NT) table[j] = 0;
    return;
  }
  const unsigned* plane = g.plane;
  unsigned* op = g.op;
  int* seg = a.ws + (long long)b * a.ws_stride;
  int* px = seg;                           // v * fw + x0 of run i
  int* xe = seg + a.max_runs;              // x1 of run i
  int* parent = COMP_LDS ? comp_smem : seg + 2 * (long long)a.max_runs;
  int* area = seg + (COMP_LDS ? 2 : 3) * (long long)a.max_runs;   // area of a root; after the choice its tag
  int* rs = seg + 4 * (long long)a.max_runs;                       // [H + 1]
  const int fw = g.fw;

  // 1  count
  // wave w owns the items [w0, w1), a contiguous range, and takes them 64 at a time, lane by lane
  const int items = g.H * g.nw, lane = tid & 63;
  const int ipw = ((items + COMP_NW - 1) / COMP_NW + 63) & ~63;
  const int w0 = min(items, (tid >> 6) * ipw), w1 = min(items, w0 + ipw);
  int mine = 0;
  for (int it = w0 + lane; it < w1; it += 64) {
    const CompItem i = comp_item(g, plane, it);
    mine += __popc(i.x & ~((i.x << 1) | i.carry));
  }
  int runs;
  const int base = comp_scan(mine, red, &runs);   // (of lane 0: the runs before the wave's first item)
  if (runs > a.max_runs) {                 // (uniform) refused: nothing was indexed by a run
    if (op) for (int j = tid; j < g.nwords; j += COMP_NT) op[j] = 0u;
    if (stats && tid < 8) stats[tid] = tid == 0 ? -1 : tid == 1 ? runs : 0;
    if (table) for (int j = tid; j < a.maxc * 5; j += COMP_NT) table[j] = 0;
    return;
  }
  // 2  list
  {
    int before = __shfl(base, 0);            // runs before the 64 items of this step
    for (int step = w0; step < w1; step += 64) {   // (uniform bounds: every lane takes part in the scan)
      const int it = step + lane;
      unsigned starts = 0u, ends = 0u;
      CompItem i = {};
      if (it < w1) {
        i = comp_item(g, plane, it);
        starts = i.x & ~((i.x << 1) | i.carry); ends = i.x & ~((i.x >> 1) | (i.next << 31));
      }
      const int cnt = __popc(starts), incl = comp_wave_scan(cnt);
      int si = before + incl - cnt;
      before += __shfl(incl, 63);
      if (it < w1 && i.wc == 0) rs[i.v] = si;
      int ei = si - (int)(i.carry & i.x & 1u);
      while (starts) {
        const int p = __ffs((int)starts) - 1;
        starts &= starts - 1u;
        px[si] = i.v * fw + i.wc * 32 + p; parent[si] = si; area[si] = 0;
        ++si;
      }
      while (ends) {
        const int q = __ffs((int)ends) - 1;
        ends &= ends - 1u;
        xe[ei++] = i.wc * 32 + q;
      }
    }
    if (tid == 0) rs[g.H] = runs;
  }
  __syncthreads();
  // 3  join
  for (int i = tid; i < runs; i += COMP_NT) {
    const int p = px[i], v = p / fw;
    if (v == 0) continue;
    const int x0 = p - v * fw, x1 = xe[i];
    const int lo = x0 - a.conn8, hi = x1 + a.conn8, e = rs[v];
    int l = rs[v - 1], r = e;              // the first run of the row above that ends at or beyond lo
    while (l < r) {
      const int m = (l + r) >> 1;
      if (xe[m] < lo) l = m + 1; else r = m;
    }
    const int above = (v - 1) * fw;
    for (int j = l; j < e && px[j] - above <= hi; ++j) comp_unite(parent, i, j);
  }
  __syncthreads();
  // 4  flatten
  int area_in = 0;
  for (int i = tid; i < runs; i += COMP_NT) {
    int r = i, p = comp_ld(parent + r);
    while (p != r) { r = p; p = comp_ld(parent + r); }
    const int p0 = px[i], v = p0 / fw, len = xe[i] - (p0 - v * fw) + 1;
    atomicAdd(area + r, len);
    area_in += len;
    if (r != i) atomicMin(parent + i, r);  // (only ever towards the root: a find that passes here meanwhile still ends at it)
  }
  area_in = comp_reduce<COMP_SUM>(area_in, red);
  // 5  choose
  const int rpt = (runs + COMP_NT - 1) / COMP_NT;
  const int r0 = min(runs, tid * rpt), r1 = min(runs, r0 + rpt);
  int nroots = 0, best_area = -1, best_root = 0x7fffffff;
  for (int i = r0; i < r1; ++i) {
    if (parent[i] != i) continue;
    ++nroots;
    const int ar = area[i];
    if (ar >= a.min_area && ar > best_area) { best_area = ar; best_root = i; }
  }
  int n;
  const int label0 = comp_scan(nroots, red, &n);
  int best = -1;
  if (a.largest) {
    const int top = comp_reduce<COMP_MAX>(best_area, red);
    best = comp_reduce<COMP_MIN>(best_area == top && top >= 0 ? best_root : 0x7fffffff, red);
  }
  const int nrows = table ? min(n, a.maxc) : 0;
  int n_kept = 0, area_out = 0;
  {
    int label = label0;
    for (int i = r0; i < r1; ++i) {
      if (parent[i] != i) continue;
      ++label;
      const int ar = area[i];
      const bool keep = ar >= a.min_area && (!a.largest || i == best);
      if (keep) { ++n_kept; area_out += ar; }
      if (label <= nrows) {                // area, xmin, y, xmax, ymax until the last pass; y is the row of the root
        int* row = table + (label - 1) * 5;
        row[0] = ar; row[1] = 0x7fffffff; row[2] = px[i] / fw; row[3] = -1; row[4] = -1;
      }
      area[i] = label | (keep ? (int)0x80000000u : 0);
    }
  }
  if (table) for (int j = nrows * 5 + tid; j < a.maxc * 5; j += COMP_NT) table[j] = 0;
  n_kept = comp_reduce<COMP_SUM>(n_kept, red);
  area_out = comp_reduce<COMP_SUM>(area_out, red);
  __syncthreads();                         // (the table rows a thread began are plain stores of this workgroup: ordered before the atomics below)
  // 6  write
  int xmin = 0x7fffffff, xmax = -1, ymin = 0x7fffffff, ymax = -1;
  if (stats || nrows > 0) {
    for (int i = tid; i < runs; i += COMP_NT) {
      const int tag = area[parent[i]], label = tag & 0x7fffffff;
      if (tag >= 0 && label > nrows) continue;
      const int p0 = px[i], v = p0 / fw, x0 = p0 - v * fw, x1 = xe[i];
      if (label <= nrows) {
        int* row = table + (label - 1) * 5;
        atomicMin(row + 1, x0); atomicMax(row + 3, x1); atomicMax(row + 4, v);
      }
      if (tag < 0) { xmin = min(xmin, x0); xmax = max(xmax, x1); ymin = min(ymin, v); ymax = max(ymax, v); }
    }
  }
  if (op) {
    for (int j = tid; j < g.nwords; j += COMP_NT) {
      unsigned x = 0u;
      int gi = j * 32, filled = 0;                          // gi: the pixel index at which the next piece begins (< 2^20 + 32)
      while (filled < 32) {
        const int v = gi / g.W, col = gi - v * g.W;
        if (v >= g.H) break;                               // past the plane's last row: the tail bits stay zero
        const int nb = min(32 - filled, g.W - col);         // bits of row v in this word: columns [col, col + nb)
        if (col < fw) {
          const int e = rs[v + 1], above = v * fw;
          int l = rs[v], r = e;                            // the first run of row v that ends at or beyond col
          while (l < r) {
            const int m = (l + r) >> 1;
            if (xe[m] < col) l = m + 1; else r = m;
          }
          for (int q = l; q < e; ++q) {
            const int x0 = px[q] - above;
            if (x0 >= col + nb) break;
            if (area[parent[q]] >= 0) continue;            // not kept
            const int c0 = max(x0, col) - col, c1 = min(xe[q], col + nb - 1) - col;   // 0 <= c0 <= c1 < nb
            const unsigned span = c1 - c0 + 1 >= 32 ? ~0u : ((1u << (c1 - c0 + 1)) - 1u) << c0;
            x |= span << filled;
          }
        }
        filled += nb; gi += nb;
      }
      op[j] = x;
    }
  }
  if (stats) {
    xmin = comp_reduce<COMP_MIN>(xmin, red); xmax = comp_reduce<COMP_MAX>(xmax, red);
    ymin = comp_reduce<COMP_MIN>(ymin, red); ymax = comp_reduce<COMP_MAX>(ymax, red);
    if (tid == 0) {
      const bool any = xmax >= 0;
      stats[0] = n; stats[1] = n_kept; stats[2] = area_in; stats[3] = area_out;
      stats[4] = any ? xmin : 0; stats[5] = any ? ymin : 0; stats[6] = any ? xmax - xmin + 1 : 0; stats[7] = any ? ymax - ymin + 1 : 0;
    }
  }
  if (nrows > 0) {                         // xmin, y, xmax, ymax -> x, y, w, h
    __syncthreads();
    for (int j = tid; j < nrows; j += COMP_NT) {
      int* row = table + j * 5;
      const int x = comp_ld(row + 1), y = row[2], x1 = comp_ld(row + 3), y1 = comp_ld(row + 4);
      row[3] = x1 - x + 1; row[4] = y1 - y + 1;
    }
  }
}
}  // namespace

extern "C" {

size_t la3d_components_workspace_bytes(int B, int H, int max_runs) {
  if (B <= 0 || H <= 0 || max_runs <= 0) return 0;
  return (size_t)B * (16 * (size_t)max_runs + 8 * (size_t)H);
}

int la3d_components_bits(const la3d_components_args* args) {
  const char* who = "la3d_components_bits";
  if (!args || args->struct_size != (int32_t)sizeof(la3d_components_args)) return refuse(who, "NULL block or bad struct_size");
  const la3d_components_args& g = *args;
  if (g.B < 0 || g.H <= 0 || g.W <= 0) return refuse(who, "bad argument (B >= 0, H, W > 0)");
  if (g.frame_width < 0 || g.frame_width > g.W) return refuse(who, "frame_width must lie in [0, W] (0 = W)");
  if (g.connectivity != 4 && g.connectivity != 8) return refuse(who, "connectivity must be 4 or 8");
  if (g.largest != 0 && g.largest != 1) return refuse(who, "largest must be 0 or 1");
  if (g.min_area < 0) return refuse(who, "min_area must not be negative");
  if (g.max_runs < 1) return refuse(who, "max_runs must be at least 1");
  if (g.max_components < 0) return refuse(who, "max_components must not be negative");
  if (g.components && g.max_components == 0) return refuse(who, "components needs max_components > 0");
  if (!g.out_bits && !g.stats && !g.components) return refuse(who, "nothing to do: out_bits, stats and components are all NULL");
  if ((long long)g.H * g.W > 1048576) return refuse(who, "H * W must not exceed 1048576", LA3D_ERR_UNSUPPORTED);
  if (g.max_runs > COMP_MAX_RUNS) return refuse(who, "max_runs must not exceed 524288 (a plane of 1048576 pixels has no more)", LA3D_ERR_UNSUPPORTED);
  if (g.B == 0) return LA3D_SUCCESS;
  if (!g.mask_bits || !g.workspace) return refuse(who, "mask_bits and workspace must not be NULL");
  if ((at(g.mask_bits) | at(g.out_bits) | at(g.stats) | at(g.components) | at(g.workspace)) & 3)
    return refuse(who, "mask_bits, out_bits, stats, components or workspace not a 4-byte aligned pointer");
  const long long words = (long long)la3d_mask_bits_words(g.H, g.W);
  const long long stride = g.bits_plane_stride ? g.bits_plane_stride : words;
  const long long out_stride = g.out_plane_stride ? g.out_plane_stride : words;
  if (stride < words) return refuse(who, "bits_plane_stride is smaller than la3d_mask_bits_words(H, W)");
  if (g.out_bits) {
    if (out_stride < words) return refuse(who, "out_plane_stride is smaller than la3d_mask_bits_words(H, W)");
    // a word of the output is gathered from runs listed before: the call does not work in place
    if (planes_overlap(g.mask_bits, (uintptr_t)g.B * (uintptr_t)stride, g.out_bits, (uintptr_t)g.B * (uintptr_t)out_stride))
      return refuse(who, "the input planes and the output planes overlap");
  }
  CompArgs a = {};
  a.bits = g.mask_bits; a.stride = stride; a.out = g.out_bits; a.out_stride = out_stride;
  a.H = g.H; a.W = g.W; a.fw = g.frame_width ? g.frame_width : g.W; a.nw = (a.fw + 31) / 32; a.nwords = (int)words;
  a.conn8 = g.connectivity == 8; a.min_area = g.min_area; a.largest = g.largest; a.max_runs = g.max_runs;
  a.maxc = g.components ? g.max_components : 0;
  a.stats = g.stats; a.comps = g.components;
  a.ws = static_cast<int*>(g.workspace); a.ws_stride = 4 * (long long)g.max_runs + 2 * (long long)g.H;
  hipStream_t st = static_cast<hipStream_t>(g.stream);
  if (g.max_runs <= COMP_LDS_RUNS) {
    allow_big_lds(reinterpret_cast<const void*>(components_kernel<true, false>));
    hipLaunchKernelGGL((components_kernel<true, false>), dim3((unsigned)g.B), dim3(COMP_NT), (size_t)g.max_runs * sizeof(int), st, a, FramesPlanes{});
  } else {
    hipLaunchKernelGGL((components_kernel<false, false>), dim3((unsigned)g.B), dim3(COMP_NT), 0, st, a, FramesPlanes{});
  }
  return check_launch("components_kernel");
}

int la3d_components_bits_frames(const la3d_components_frames_args* args) {
  const char* who = "la3d_components_bits_frames";
  if (!args || args->struct_size != (int32_t)sizeof(la3d_components_frames_args)) return refuse(who, "NULL block or bad struct_size");
  const la3d_components_frames_args& g = *args;
  if (g.B < 0 || g.P < 0 || g.H <= 0 || g.W <= 0) return refuse(who, SIZES_FRAMES);
  if (g.connectivity != 4 && g.connectivity != 8) return refuse(who, "connectivity must be 4 or 8");
  if (g.largest != 0 && g.largest != 1) return refuse(who, "largest must be 0 or 1");
  if (g.min_area < 0) return refuse(who, "min_area must not be negative");
  if (g.max_runs < 1) return refuse(who, "max_runs must be at least 1");
  if (g.max_components < 0) return refuse(who, "max_components must not be negative");
  if (g.components && g.max_components == 0) return refuse(who, "components needs max_components > 0");
  if (!g.out_bits && !g.stats && !g.components) return refuse(who, "nothing to do: out_bits, stats and components are all NULL");
  if (g.reserved[0] != 0 || g.reserved[1] != 0) return refuse(who, "reserved must be 0");
  if (g.bits_words < 0 || (g.out_bits && g.out_words < 0)) return refuse(who, "bits_words and out_words must not be negative");
  if ((at(g.bits) | at(g.out_bits)) & 15) return refuse(who, "bits or out_bits not a 16-byte aligned pointer");
  if ((at(g.bits_offsets) | at(g.out_offsets) | at(g.frames)) & 7) return refuse(who, "bits_offsets, out_offsets or frames not an 8-byte aligned pointer");
  if ((at(g.stats) | at(g.components) | at(g.workspace) | at(g.image_index)) & 3)
    return refuse(who, "stats, components, workspace or image_index not a 4-byte aligned pointer");
  // a word of the output is gathered from runs listed before: the call does not work in place
  if (g.bits && g.out_bits && planes_overlap(g.bits, (uintptr_t)g.bits_words, g.out_bits, (uintptr_t)g.out_words))
    return refuse(who, "the input buffer and the output buffer overlap");
  if (g.B > 0) {
    if (!g.bits || !g.bits_offsets || !g.image_index || !g.workspace || (!g.frames && g.P > 0))
      return refuse(who, "NULL bits, bits_offsets, image_index, workspace or frames");
    if (g.out_bits && !g.out_offsets) return refuse(who, "out_offsets must not be NULL with out_bits");
  }
  if (bounds_words(g.H, g.W) * 32 > 1048576)
    return refuse(who, "the bounds' H * roundup32(W) must not exceed 1048576", LA3D_ERR_UNSUPPORTED);
  if (g.max_runs > COMP_MAX_RUNS) return refuse(who, "max_runs must not exceed 524288 (a plane of 1048576 pixels has no more)", LA3D_ERR_UNSUPPORTED);
  if (g.B == 0) return LA3D_SUCCESS;
  CompArgs a = {};
  a.bits = g.bits; a.out = g.out_bits;
  a.H = g.H; a.W = g.W;                      // the bounds: every other word of a plane's geometry is formed per workgroup
  a.conn8 = g.connectivity == 8; a.min_area = g.min_area; a.largest = g.largest; a.max_runs = g.max_runs;
  a.maxc = g.components ? g.max_components : 0;
  a.stats = g.stats; a.comps = g.components;
  a.ws = static_cast<int*>(g.workspace); a.ws_stride = 4 * (long long)g.max_runs + 2 * (long long)g.H;
  FramesPlanes fr = {};
  fr.offsets = reinterpret_cast<const long long*>(g.bits_offsets); fr.out_offsets = reinterpret_cast<const long long*>(g.out_offsets);
  fr.frames = g.frames; fr.image_index = g.image_index; fr.P = g.P;   // (P == 0: every row is refused before a frame row is addressed)
  fr.bits_words = g.bits_words; fr.out_words = g.out_bits ? g.out_words : 0;
  hipStream_t st = static_cast<hipStream_t>(g.stream);
  if (g.max_runs <= COMP_LDS_RUNS) {
    allow_big_lds(reinterpret_cast<const void*>(components_kernel<true, true>));
    hipLaunchKernelGGL((components_kernel<true, true>), dim3((unsigned)g.B), dim3(COMP_NT), (size_t)g.max_runs * sizeof(int), st, a, fr);
  } else {
    hipLaunchKernelGGL((components_kernel<false, true>), dim3((unsigned)g.B), dim3(COMP_NT), 0, st, a, fr);
  }
  return check_launch("components_kernel");
}

}  // extern "C"
