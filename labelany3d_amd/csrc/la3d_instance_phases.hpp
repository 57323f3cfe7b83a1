// la3d_instance_phases.hpp - the phases of fit_instances_kernel (la3d_instance.hip) between the depth walks (la3d_walks.hpp) and the
// axis / box stages (la3d_stages.hpp): mask -> bit image, the fused keep rule, the active-tile list, the
// rank-select of the subsample mode and the header of a hull hand-off.  Every thread of the workgroup calls a phase; what a phase
// leaves in LDS is visible after the barrier its caller passes next.  tid arrives by value: the caller decides whether it is the
// kernel's input register or rebuilt from wave and lane (tid_here).
#pragma once
#include "la3d_device.hpp"
#include "la3d_poly.hpp"
#include "la3d_hull.hpp"

using namespace la3d;

namespace {
// ---- phase 0: the mask of instance inst -> bit image in LDS; returns this thread's share of the mask's pixel count ----
// SRC as in fit_instances_kernel.  p: the workgroup's parameters, call: the kernel argument (they differ in a frames call).
// stage / stage_words: the LDS behind Shared - the tile list's, which is built afterwards -, borrowed by the decoders.
template <bool VEC, int SRC, bool FRAMES>
__device__ inline int mask_to_bits(const FitParams& p, const FitParams& call, int inst, const unsigned char* mpl, unsigned* bits, Shared* sh,
                                   void* stage, int stage_words, int tid, int wave, int lane) {
  const int HW = p.HW;
  int nmask = 0;
  if constexpr (SRC == 1) {
    // masks arrive as COCO run lengths: decode straight into the LDS bit image — no u8 plane is ever read
    // (the block totals of the column scan go through the stage)
    const long long o0 = p.rle_offsets[inst];
    nmask = rle_to_bits<NT>(p.rle_counts + o0, (int)(p.rle_offsets[inst + 1] - o0), bits, p.nwords, p.H, p.W, sh->scan, tid,
                            static_cast<unsigned*>(stage), stage_words, p.frame_w);
  } else if constexpr (SRC == 2) {
    // masks arrive as polygon parts (the reference's create_boolean_mask_from_polygon, src/util.py:386-400): rasterised with
    // cv2.fillPoly's rule straight into the LDS bit image; the sides go through the stage
    nmask = poly_to_bits<NT>(p.poly_xy, p.poly_ring_off, p.poly_inst_rings[inst], p.poly_inst_rings[inst + 1],
                             static_cast<PolySide*>(stage), sh->scan, bits, p.nwords, p.H, p.W, tid, p.frame_w);
  } else if constexpr (SRC == 3) {
    // masks arrive as bit planes: the plane IS the bit image - a straight stream into LDS, no decode (38 400 B for 640x480 against
    // the 307 200 B of a u8 plane)
    // (frames call: the plane lies at its own offset - accepted by the caller, loaded again here -, holds the whole words of the
    // instance's own frame and is 16-byte aligned: always the 16-byte form)
    if constexpr (FRAMES) nmask = bits_plane_to_lds<NT>(p.mask_bits + frame_bits_offset(call, inst), bits, p.nwords, HW, 1, tid);
    else nmask = bits_plane_to_lds<NT>(p.mask_bits + (long long)inst * p.bits_plane_stride, bits, p.nwords, HW, p.bits_vec, tid);
  } else {
    unsigned short* b16 = reinterpret_cast<unsigned short*>(bits);
    const int ngroups = (HW + 15) >> 4;
    if (VEC) {
      const u32x4* m4 = reinterpret_cast<const u32x4*>(mpl);
      // Optimistic form: np.bool_ planes (the reference's layout, src/util.py:367,382) hold only 0 and 1, and then the
      // 16-bit pattern of a 16-byte group is four dot products (sum byte_j * 2^j) - 11 VALU instructions per group instead
      // of 27 for the general non-zero test.  Every word is ORed into `seen`; a byte above 1 anywhere in the plane sends the
      // whole workgroup through the general loop below (same bit image either way).
      constexpr int P0U = 4;   // 16-byte loads in flight per lane
      unsigned seen = 0;
#pragma unroll P0U
      for (int g = tid; g < ngroups; g += NT) {
        const u32x4 w = __builtin_nontemporal_load(m4 + g);
        const unsigned lo = __builtin_amdgcn_udot4(w.y, 0x80402010u, __builtin_amdgcn_udot4(w.x, 0x08040201u, 0u, false), false);
        const unsigned hi = __builtin_amdgcn_udot4(w.w, 0x80402010u, __builtin_amdgcn_udot4(w.z, 0x08040201u, 0u, false), false);
        const unsigned pat = lo | (hi << 8);
        seen |= (w.x | w.y) | (w.z | w.w);
        b16[g] = (unsigned short)pat;
        nmask += __popc(pat);
      }
      const unsigned long long odd = __ballot((seen & 0xfefefefeu) != 0);
      if (lane == 0) sh->scan[wave] = odd != 0 ? 1u : 0u;
      __syncthreads();
      unsigned general = 0;
#pragma unroll
      for (int w = 0; w < NWAVE; ++w) general |= sh->scan[w];
      if (general) {   // uniform: some byte is neither 0 nor 1 (e.g. 255-valued masks)
        nmask = 0;
#pragma unroll 4
        for (int g = tid; g < ngroups; g += NT) {
          const u32x4 w = m4[g];
          const unsigned pat = nz16(w.x, w.y, w.z, w.w);
          b16[g] = (unsigned short)pat;
          nmask += __popc(pat);
        }
      }
    } else {
      for (int g = tid; g < ngroups; g += NT) {
        unsigned pat = 0;
        for (int k = 0; k < 16; ++k) {
          const int i = g * 16 + k;
          if (i < HW && mpl[i]) pat |= 1u << k;
        }
        b16[g] = (unsigned short)pat;
        nmask += __popc(pat);
      }
    }
    if ((ngroups & 1) && tid == 0) b16[ngroups] = 0;  // upper half of the last 32-bit word
  }
  return nmask;
}

// ---- the fused keep rule: the reference's instance filter (src/util.py:375) on the bit image just built.  Returns keep; a dropped
// instance (LA3D_BOX_FILTERED, aux[2] = the mask's area) has its outputs written here and costs no passes ----
template <int SRC>
__device__ inline bool filter_keep(const FitParams& p, Shared* sh, const unsigned* bits, int inst, int tid) {
  int st4[4];
  bits_filter_stats<NT>(bits, p.H, p.frame_w, p.filter_boundary, reinterpret_cast<int*>(sh->part), tid, st4, p.W);   // (frame_w == W unless the rows are padded)
  if (p.filter_stats && tid < 4) (p.filter_stats + (long long)inst * 4)[tid] = st4[tid];   // (uniform base: scalar address arithmetic)
  // run lengths: rows holding a pixel (:368-369); polygons: last - first + 1 (:328-335); a bit plane does not say where it came from: the caller's flag
  const int height = SRC == 1 ? st4[1] : (SRC == 3 && !p.bits_span) ? st4[1] : st4[2];
  const bool keep = 16 * height > p.H && st4[3] < p.filter_max_edge && st4[0] >= p.filter_min_area;   // height / H > 0.0625
  if (!keep && tid == 0) write_no_box(p, inst, LA3D_BOX_FILTERED, 0.0, (double)st4[0]);
  return keep;
}

// ---- active-tile list (deterministic two-pass compaction: count, prefix, write) ----
// nactive: entries of list (-1: more than p.list_cap - the dense walk), nfull: how many of them lie completely inside the mask (they
// come first).  LK (the plain tiled build): compact - the bit image has been compacted to the active tiles (eight row words per
// list entry) and the LDS that frees keeps depth tiles between the passes (sweep_tiled); sep - the instance takes the separable
// single pass (sweep_sep), its per-column depth ranges initialised behind the entries.
struct TileList {
  int nactive = 0, nfull = 0, compact = 0;
  bool sep = false;
};

// one wave's look at up to 4 x 64 tiles: the ballots of the active tiles (bal), how many are active / full, bit k of fl: this lane's
// k-th tile lies completely inside the mask (all eight row words all ones); LK: the eight row words of the lane's tiles (wrd).
// WHOLE_ROWS: every tile row is complete (H % 8 == 0: the common frame heights) - no row clamp, no select per word; otherwise rows
// past the frame re-read the last one and are stored as zeros (never "full").  No integer division.
template <bool WHOLE_ROWS, bool LK>
__device__ inline void classify_tiles(const FitParams& p, const unsigned* bits, int tbeg, int tend, int lane, unsigned long long* bal,
                                      unsigned (*wrd)[8], int* wcount, int* fcount, unsigned* fl) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = tbeg + k * 64 + lane;
    unsigned any = 0, all = 0xffffffffu;
    if (t < tend) {
      const int ty = (int)(((float)t + 0.5f) * p.rcp_ntx), tx = t - ty * p.ntx;  // exact: see instance_fit
      const int rmax = p.H - 1 - ty * 8;                                        // >= 0
      const unsigned* bw = bits + (ty * 8) * p.ntx + tx;
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const unsigned w = bw[(WHOLE_ROWS ? rr : min(rr, rmax)) * p.ntx];
        any |= w;
        if constexpr (LK) { wrd[k][rr] = (WHOLE_ROWS || rr <= rmax) ? w : 0u; all &= wrd[k][rr]; }
      }
    }
    bal[k] = __ballot(any != 0);
    *wcount += __popcll(bal[k]);
    if constexpr (LK) {
      const bool f = t < tend && all == 0xffffffffu;
      *fcount += __popcll(__ballot(f));
      *fl |= (f ? 1u : 0u) << k;
    }
  }
}

template <bool LK>
__device__ inline TileList build_tile_list(const FitParams& p, Shared* sh, unsigned* bits, unsigned short* list, bool sep_cam, int tid, int wave, int lane) {
  TileList tl;
  const int ntiles = p.ntx * p.nty, per = p.tiles_per_wave;
  const int tbeg = wave * per, tend = min(tbeg + per, ntiles);
  int base = 0;
  if (per <= 256) {
    // one pass: a wave looks at up to 4 x 64 tiles; the ballots stay in SGPRs across the barrier, the eight row words
    // of a tile are read back to back
    unsigned long long bal[4];
    unsigned wrd[LK ? 4 : 1][8];
    int wcount = 0, fcount = 0;
    unsigned fl = 0;
    if ((p.H & 7) == 0) classify_tiles<true, LK>(p, bits, tbeg, tend, lane, bal, wrd, &wcount, &fcount, &fl);   // uniform
    else classify_tiles<false, LK>(p, bits, tbeg, tend, lane, bal, wrd, &wcount, &fcount, &fl);
    if (lane == 0) sh->scan[wave] = (unsigned)wcount | ((unsigned)fcount << 16);   // (at most 256 tiles per wave)
    __syncthreads();
    LA3D_SUBSTAMP(sh, 14);
    // Round 6: the list holds the tiles that lie completely inside the mask FIRST ([0, nfull): the separable pass walks them with
    // a body that needs no mask bits), the others behind them - each class in tile order.  Any order of the list gives a valid
    // walk; the order only decides how the fp64 partial sums are grouped.
    int fbase = 0;
    for (int w = 0; w < NWAVE; ++w) {
      const int c = (int)(sh->scan[w] & 0xffffu), f = (int)(sh->scan[w] >> 16);
      if (w < wave) { base += c - f; fbase += f; }
      tl.nactive += c;
      tl.nfull += f;
    }
    if (tl.nactive > p.list_cap) {
      tl.nactive = -1;  // uniform: every thread sees the same total
      tl.nfull = 0;
    } else {
      // (with pass-B culling the compact image also holds the survivor list / the depth ranges behind the entries)
      // every wave read its row words before the barrier above: the image region can be overwritten in place
      if constexpr (LK) tl.compact = (tl.nactive * 32 + cull_rng_words(tl.nactive) * 4 <= p.mask_lds_bytes) ? 1 : 0;   // uniform
      int foff = fbase, poff = tl.nfull + base;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool isf = LK && ((fl >> k) & 1u);
        const unsigned long long bf = LK ? __ballot(isf) : 0ull, bp = bal[k] & ~bf, lt = (1ull << lane) - 1ull;
        if ((bal[k] >> lane) & 1ull) {
          const int t = tbeg + k * 64 + lane;
          const int ty = (int)(((float)t + 0.5f) * p.rcp_ntx), tx = t - ty * p.ntx;
          const int idx = isf ? foff + __popcll(bf & lt) : poff + __popcll(bp & lt);
          list[idx] = (unsigned short)((ty << 8) | tx);
          if constexpr (LK) if (tl.compact) {   // uniform
            uint4* e = reinterpret_cast<uint4*>(bits) + 2 * idx;
            e[0] = make_uint4(wrd[k][0], wrd[k][1], wrd[k][2], wrd[k][3]);
            e[1] = make_uint4(wrd[k][4], wrd[k][5], wrd[k][6], wrd[k][7]);
          }
        }
        foff += __popcll(bf); poff += __popcll(bp);
      }
      if constexpr (LK) if (tl.compact) {   // uniform
        if (sep_cam && tl.nactive * 32 + sep_col_words(p.W) * 4 <= p.mask_lds_bytes) {   // uniform
          tl.sep = true;   // per-column depth range behind the entries: [min | max], the identities of unsigned min / max
          unsigned* col = bits + tl.nactive * 8;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
          for (int u = tid; u < p.W; u += NT) { col[u] = 0xffffffffu; col[p.W + u] = 0u; }
        }
      }
    }
  } else {
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
      int wcount = 0;
      for (int t0 = tbeg; t0 < tend; t0 += 64) {   // wave-uniform trip count
        const int t = t0 + lane;
        unsigned any = 0, packed = 0;
        if (t < tend) {
          const int ty = t / p.ntx, tx = t - ty * p.ntx;
          const int rows = min(8, p.H - ty * 8);
          const unsigned* bw = bits + (ty * 8) * p.ntx + tx;
          for (int rr = 0; rr < rows; ++rr) any |= bw[rr * p.ntx];
          packed = ((unsigned)ty << 8) | (unsigned)tx;
        }
        const unsigned long long bal = __ballot(any != 0);
        if (pass == 1 && any) list[base + wcount + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)packed;
        wcount += __popcll(bal);
      }
      if (pass == 0) {
        if (lane == 0) sh->scan[wave] = (unsigned)wcount;
        __syncthreads();
        for (int w = 0; w < NWAVE; ++w) {
          const int c = (int)sh->scan[w];
          if (w < wave) base += c;
          tl.nactive += c;
        }
        if (tl.nactive > p.list_cap) { tl.nactive = -1; break; }  // uniform: every thread sees the same total
      }
    }
  }
  return tl;
}

// ---- reference-subsample mode: the rank-select.  Thread t < 500 finds the pixel whose rank among the ntot mask pixels is its drawn
// index (hull call with ntot <= 500: its own index - every pixel once) and leaves it as a point of the ground-aligned frame in
// px / py / pz / pok, with its first moments in acc / cnt (all unchanged for a thread without a point; a non-finite depth: pok
// false, the point three zeros) ----
template <bool HULL, bool FRAMES, typename DepthT>
__device__ inline void sample_pick(const FitParams& p, Shared* sh, const unsigned* bits, unsigned* prefix, const DepthT* __restrict__ dpl,
                                          const DepthCvt<DepthT> cv, const double* Mg, int ntot, int my_draw, int tid, int wave, int lane,
                                          double* acc, int* cnt, double* ppx, double* ppy, double* ppz, bool* ppok) {
  // exclusive prefix of the popcounts of 32-word blocks (1024 px): thread t owns block t.  One word of LDS per block
  // keeps the workgroup at a quarter of the CU's LDS (four workgroups per CU, like the full-mask build).
  const int nblk = (p.nwords + 31) >> 5;
  unsigned run0 = 0;   // blocks of earlier rounds (frames above NT * 1024 px)
  for (int b0 = 0; b0 < nblk; b0 += NT) {
    const int blk = b0 + tid;
    unsigned local = 0;
    if (blk < nblk) {
      const int w0 = blk << 5, wn = min(32, p.nwords - w0);
      if (wn == 32) {
        const uint4* q = reinterpret_cast<const uint4*>(bits + w0);
#pragma unroll
        for (int i = 0; i < 8; ++i) { const uint4 v = q[i]; local += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w); }
      } else {
        for (int i = 0; i < wn; ++i) local += __popc(bits[w0 + i]);
      }
    }
    unsigned incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (lane == 63) sh->scan[wave] = incl;
    __syncthreads();
    unsigned base = run0, tot = 0;
    for (int w = 0; w < NWAVE; ++w) { const unsigned c = sh->scan[w]; if (w < wave) base += c; tot += c; }
    if (blk < nblk) prefix[blk] = base + incl - local;
    run0 += tot;
    __syncthreads();
  }
  if (tid < (HULL ? min(ntot, LA3D_NSAMPLE) : LA3D_NSAMPLE)) {
    int r = (HULL && ntot <= LA3D_NSAMPLE) ? tid : my_draw;
    r = r < 0 ? 0 : (r >= ntot ? ntot - 1 : r);
    int lo = 0, hi = nblk - 1;
    while (lo < hi) {  // last block whose exclusive prefix is <= r
      const int mid = (lo + hi + 1) >> 1;
      if (prefix[mid] <= (unsigned)r) lo = mid; else hi = mid - 1;
    }
    int k = r - (int)prefix[lo];          // rank inside the block
    lo <<= 5;
    unsigned w = 0;
    if (lo + 32 <= p.nwords) {
      // the word of the block that holds set bit k: all 32 words read at once, then a register scan
      uint4 q[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) q[i] = reinterpret_cast<const uint4*>(bits + lo)[i];
      int sel = 0;
      bool found = false;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        const unsigned wi = (i & 3) == 0 ? q[i >> 2].x : (i & 3) == 1 ? q[i >> 2].y : (i & 3) == 2 ? q[i >> 2].z : q[i >> 2].w;
        const int c = __popc(wi);
        const bool here = !found && k < c;
        if (here) { w = wi; sel = i; }
        found = found || here;
        if (!found) k -= c;
      }
      lo += sel;
    } else {
      const int wend = p.nwords - 1;
      for (; lo < wend; ++lo) {
        const int c = __popc(bits[lo]);
        if (k < c) break;
        k -= c;
      }
      w = bits[lo];
    }
    for (; k > 0; --k) w &= w - 1;  // drop k lowest set bits
    const unsigned i = (unsigned)lo * 32u + (unsigned)(__ffs((int)w) - 1);
    const float df = depth_at<DepthT>(dpl, i, cv);
    unsigned u, v;
    // (frames call: the workgroup's copy of the parameters still holds the rcpW of the call's bounds - see frame_geometry)
    pix_uv(i, p.W, FRAMES ? 1.0f / (float)p.W : p.rcpW, &u, &v);
    const double ud = (double)u, vd = (double)v;
    const bool pok = finite_f32(df);
    const double d = pok ? (double)df : 0.0;
    const double px = d * fma(Mg[0], ud, fma(Mg[1], vd, Mg[2]));
    const double py = d * fma(Mg[3], ud, fma(Mg[4], vd, Mg[5]));
    const double pz = d * fma(Mg[6], ud, fma(Mg[7], vd, Mg[8]));
    *ppx = px; *ppy = py; *ppz = pz; *ppok = pok;
    if (pok) {
      acc[0] = px; acc[1] = pz; acc[2] = px * px; acc[3] = px * pz; acc[4] = pz * pz;
      *cnt = 1;
    }
  }
}

// ---- the header of a hull hand-off (la3d_hull.hpp: HH_*), ONE thread: what the axis stage left in Shared, the y extent and the
// column rays of the full-mask mode (zeros in the subsample mode), the number of handed-over points (0 in the full-mask mode); the
// state last: 0 = to be finished by hull_finish_kernel ----
__device__ inline void hull_handoff_header(double* hh, const Shared* sh, double ylo, double yhi, double a00, double a02, double npts) {
  hh[HH_NVALID] = (double)sh->n_valid; hh[HH_NM] = (double)sh->nm; hh[HH_CYAW] = sh->cyaw; hh[HH_SYAW] = sh->syaw;
  hh[HH_GAP] = sh->gap; hh[HH_YLO] = ylo; hh[HH_YHI] = yhi;
  for (int i = 0; i < 9; ++i) hh[HH_RG + i] = sh->Rg[i];
  hh[HH_A00] = a00; hh[HH_A02] = a02; hh[HH_NPTS] = npts;
  hh[HH_STATE] = 0.0;
}
}  // namespace
