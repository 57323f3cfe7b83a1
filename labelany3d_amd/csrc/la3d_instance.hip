// la3d_instance.hip - the INSTANCE ENGINE of la3d_fit_instances: one 512-thread workgroup per instance (mask -> bit image in LDS ->
// active-tile list -> separable single pass, or pass A / axis / pass B -> record), its launch order helper kernel and its launcher.
// Design and measurements: DESIGN.md section 4.1; the walks and stages it is built from: la3d_walks.hpp, la3d_stages.hpp.
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
#include "la3d_engines.hpp"
#include "la3d_walks.hpp"
#include "la3d_stages.hpp"
#include "la3d_hull.hpp"

// This file is compiled three times: as itself for float32 depth planes, and - included by la3d_instance_f16.hip /
// la3d_instance_u16.hip, which set LA3D_INSTANCE_DT - for the 16-bit planes of la3d_fit_instances_depth16 (translation units of
// their own: they compile side by side with this one).  Everything that differs sits behind DepthT / KParams / the DepthCvt the
// walks take; with LA3D_INSTANCE_DT == 0 the kernels are the ones they were.
#ifndef LA3D_INSTANCE_DT
#define LA3D_INSTANCE_DT 0
#endif
#if LA3D_INSTANCE_DT == 0
using DepthT = float;
using KParams = la3d::FitParams;
#define LA3D_INSTANCE_FIT instance_fit
#elif LA3D_INSTANCE_DT == 1
using DepthT = la3d::d_f16;
using KParams = la3d::FitParams16;
#define LA3D_INSTANCE_FIT instance_fit_f16
#define fit_instances_kernel fit_instances_f16_kernel
#else
using DepthT = la3d::d_u16;
using KParams = la3d::FitParams16;
#define LA3D_INSTANCE_FIT instance_fit_u16
#define fit_instances_kernel fit_instances_u16_kernel
#endif

namespace {
// the planes of a call and what turns their elements into the float32 that is fitted
__device__ inline const float* depth_planes(const FitParams& p, const FitParams&) { return p.depth; }
__device__ inline DepthCvt<float> depth_cvt(const FitParams&) { return {}; }
#if LA3D_INSTANCE_DT != 0
__device__ inline const DepthT* depth_planes(const FitParams&, const FitParams16& call) { return reinterpret_cast<const DepthT*>(call.depth16); }
__device__ inline DepthCvt<DepthT> depth_cvt(const FitParams16& call) {
  DepthCvt<DepthT> cv;
#if LA3D_INSTANCE_DT == 2
  cv.scale = call.d16_scale; cv.hole = call.d16_hole;
#endif
  return cv;
}
// the depth_offset of a frame row that frame_geometry has accepted (wave-uniform: scalar registers).  A second load of the word
// frame_geometry checked - FitParams has no field to carry it in, and does not grow for it: the frame table is an INPUT of the call,
// which nothing writes while the call runs (include/la3d.h: frames), so both loads see the same value
__device__ inline long long frame_depth_offset(const FitParams& call, int img) {
  const long long off_v = call.frames[img].depth_offset;
  return ((long long)__builtin_amdgcn_readfirstlane((int)(off_v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)off_v);
}
#endif
// ------------------------------------------------------------------------------------------
// instance engine: one workgroup per instance
// ------------------------------------------------------------------------------------------
// SRC: where the mask comes from - 0 = u8 plane, 1 = COCO run lengths, 2 = polygon parts (both decoded into the LDS bit image),
// 3 = bit plane (la3d_fit_instances_bits: the LDS bit image itself, copied in)
// The checked separable walk of the hull instantiations (full-mask mode): what sweep_sep does - moments, y extent, per-column depth
// range in ONE walk over the compacted tile list - with a finite test per pixel (NaN / infinite depths under the mask are holes of a
// real depth map: dropped, as the reference drops them, src/util_3dbox.py:139) and range keys that order negative depths too
// (hull_key).  Moments about (px0, pz0).  col = colmin[W] | colmax[W], initialised to 0xffffffff / 0.  One tile per wave and step;
// lane = (column c of the tile, four rows from h4).
__device__ inline void sweep_sep_hull(const FitParams& p, const DepthT* __restrict__ dpl, const unsigned* bits, const unsigned short* list,
                                      int nactive, const double* Mg, unsigned* col, int wave, int lane, double px0, double pz0,
                                      double* acc, double* yext, int* cnt, const DepthCvt<DepthT> cv) {
  const int c = lane & 31, h4 = (lane >> 5) * 4;
  const double a00 = Mg[0], a02 = Mg[2], a11 = Mg[4], a12 = Mg[5];
  double s0 = acc[0], s1 = acc[1], s2 = acc[2], s3 = acc[3], s4 = acc[4], ylo = yext[0], yhi = yext[1];
  int n = *cnt;
  for (int e = wave; e < nactive; e += NWAVE) {   // wave-uniform
    const unsigned t = __builtin_amdgcn_readfirstlane((unsigned)list[e]);
    const int u = (int)(t & 0xffu) * 32 + c, v0 = (int)(t >> 8) * 8 + h4;   // u < W: the tiles cover exactly W = 32 ntx columns
    const uint4 w = *reinterpret_cast<const uint4*>(bits + e * 8 + h4);
    const unsigned nib = ((w.x >> c) & 1u) | (((w.y >> c) & 1u) << 1) | (((w.z >> c) & 1u) << 2) | (((w.w >> c) & 1u) << 3);
    const double r0 = fma(a00, (double)u, a02);
    unsigned kmin = 0xffffffffu, kmax = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = v0 + k;
      if (((nib >> k) & 1u) && v < p.H) {   // (rows past the frame carry no mask bit; the test keeps the load inside the plane regardless)
        const float df = depth_at<DepthT>(dpl, (long long)v * p.W + u, cv);
        if (finite_f32(df)) {
          const unsigned key = hull_key(__float_as_uint(df));
          kmin = min(kmin, key); kmax = max(kmax, key);
          const double d = (double)df;
          const double x = d * r0 - px0, z = d - pz0, y = d * fma(a11, (double)v, a12);
          s0 += x; s1 += z; s2 = fma(x, x, s2); s3 = fma(x, z, s3); s4 = fma(z, z, s4);
          ylo = fmin(ylo, y); yhi = fmax(yhi, y);
          n += 1;
        }
      }
    }
    if (kmin <= kmax) { atomicMin(col + u, kmin); atomicMax(col + p.W + u, kmax); }
  }
  acc[0] = s0; acc[1] = s1; acc[2] = s2; acc[3] = s3; acc[4] = s4; yext[0] = ylo; yext[1] = yhi;
  *cnt = n;
}

// HULL: the instantiations of a convex-hull call (la3d_fit_args::method) - everything a PCA call does up to
// and including the axis, then, instead of extents and record, the hand-off of hull_finish_kernel through the workspace (p.geo
// points at the call's hand-off area).  Every difference sits behind the constant HULL: the PCA instantiations (HULL = false) compile to the code they were.
// FRAMES: the instantiations of la3d_fit_instances_frames (in the 16-bit units: of la3d_fit_instances_frames_depth16) - images of
// different sizes in one call.  The kernel argument then holds the call's sizing bounds; once the workgroup knows its instance and image it reads the image's la3d_frame row and replaces the
// frame geometry in ITS copy of the parameters (frame_geometry, la3d_device.hpp), which everything below reads.  Every difference sits behind the
// constant FRAMES: the other instantiations read the kernel argument itself, as they did.
template <bool VEC, bool LDSMASK, bool SAMPLE, bool TILED, int SRC, bool HULL = false, bool FRAMES = false>
__global__ __launch_bounds__(NT, NT / 64) void fit_instances_kernel(const KParams p_call) {
  static_assert(!FRAMES || (VEC && LDSMASK && TILED && !HULL && (SRC == 1 || SRC == 2 || SRC == 3)), "frames calls: run lengths / polygons / bit planes, tiled form");
  FitParams p_frame;   // FRAMES only: this workgroup's parameters (dead otherwise)
  if constexpr (FRAMES) p_frame = p_call;
  const FitParams& p_block = p_call;
  const FitParams& p = FRAMES ? p_frame : p_block;   // (the LDS LAYOUT below is always the call's: p_call.mask_lds_bytes)
  constexpr bool RLE = SRC == 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  Shared* sh = reinterpret_cast<Shared*>(smem + p_call.mask_lds_bytes);
  unsigned* prefix = reinterpret_cast<unsigned*>(smem + p_call.mask_lds_bytes + sizeof(Shared));  // SAMPLE only
  // TILED only: compacted list of active tile ids
  unsigned short* list = reinterpret_cast<unsigned short*>(smem + p_call.mask_lds_bytes + sizeof(Shared));

  // (builds that carry the separable pass take the lane from the execution mask, not from threadIdx.x - the workgroup's waves are
  // full -, and rebuild the thread index where it is used: neither then keeps the kernel's input register alive across the passes)
  constexpr bool REBUILD_TID = TILED && !SAMPLE;
  const int tid_in = threadIdx.x;
  const int lane = REBUILD_TID ? (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) : (tid_in & 63);
  const int wave = __builtin_amdgcn_readfirstlane(tid_in >> 6);  // wave-uniform: lives in an SGPR
  const int tid = REBUILD_TID ? ((wave << 6) | lane) : tid_in;
#ifdef LA3D_TIMELINE
  const unsigned long long t_entry = wall_clock64();   // before the first memory access of the workgroup
#endif
  // (measured, profiles/timeline.py: all workgroups of a launch ENTER within 0.7 us, but VMEM issue is arbitrated by age, so the
  // youngest of the four workgroups of a CU gets its first load - this perm entry - back only when an older one has finished
  // its mask stream, ~25 us in; warming the table through L1 does not help, and s_setprio by dispatch group only moves the
  // starvation to the oldest group, which holds the largest instances: DESIGN.md section 5.2)
  // (self-estimating launch; order_self == 2 is the test mode of the fallback: every seventh workgroup keeps its key to itself)
  // (batches above one resident set: the workgroups of the FIRST set - the only ones certain to run without waiting for anybody -
  // estimate instances b, b + R, b + 2R, ...)
  if (!FRAMES && !SAMPLE && p.order_self && (int)blockIdx.x < p.order_resident && !(p.order_self == 2 && blockIdx.x % 7 == 3)) {
    for (int ie = (int)blockIdx.x; ie < p.B; ie += p.order_resident) {   // uniform
      if (ie != (int)blockIdx.x) __syncthreads();   // (the block totals of the previous estimate have been read)
      estimate_publish_wg<SRC == 3>(p, ie, sh, tid, wave, lane);
    }
  }
  const int inst = p.order_nch > 0 ? order_select<SRC == 3>(p, (int)blockIdx.x, sh, wave, lane) : xcd_remap(blockIdx.x, p.B);
  if (tid == 0) { sh->order_inst = inst; sh->sep_bad = 0; }   // (the instance is re-read after the mask stage, see below)
  if constexpr (HULL) { if (tid == 0) hull_slot(p.geo, inst, hull_stride_bytes(SAMPLE, p.W))[HH_STATE] = -1.0; }   // nothing to finish, until the hand-off says so
  const int img = p.image_index ? p.image_index[inst] : inst;
  if constexpr (FRAMES) {
    // uniform: an image index outside the table or a frame row outside the contract - refused; bit planes: so is a plane offset
    // outside its contract, loaded only behind an accepted row (frame_bits_offset)
    if (!frame_geometry<true, SAMPLE>(p_frame, p_call, img) || (SRC == 3 && !frame_bits_offset_ok(p_call, inst))) {
      if (tid == 0) {                    // before anything is read through it (no barrier has been passed: the whole workgroup leaves)
        if (p.aux) {
          double* a = p.aux + (long long)inst * LA3D_AUX;
          a[0] = NAN; a[1] = 0.0; a[2] = NAN; a[3] = NAN;
        }
        p.status[inst] = LA3D_BOX_UNSUPPORTED;
        write_nan_box(p.out + (long long)inst * LA3D_REC);
        if (p.proj) { for (int j = 0; j < 8; ++j) p.proj[(long long)inst * 8 + j] = NAN; }
      }
      return;
    }
  }
  const int HW = p.HW;
  const DepthT* dpl = depth_planes(p, p_call) + (long long)img * p.depth_plane_stride;
#if LA3D_INSTANCE_DT != 0
  // frames call on 16-bit planes (la3d_fit_instances_frames_depth16): depth_planes() is the base of the ragged buffer and the frame
  // row's depth_offset - which has passed frame_geometry's check above: >= 0, % 4 == 0, so the plane is 8-byte aligned - counts
  // ELEMENTS of it (frame_geometry left depth_plane_stride 0; its p.depth is not read in these units)
  if constexpr (FRAMES) dpl += frame_depth_offset(p_call, img);
#endif
  const DepthCvt<DepthT> cv = depth_cvt(p_call);
  const unsigned char* mpl = p.mask ? p.mask + (long long)inst * HW : nullptr;

  if (tid == NT - 1) {
    // per-instance geometry (reference src/util.py:56, src/util_3dbox.py:128-134), one lane, overlapped with the
    // mask stream of everyone else: Kinv, Rg, M = Rg^T Kinv
    double Kinv[9], Rg[9];
    inv3_camera(p.K + (long long)img * p.k_stride, Kinv);
    sh->bad_ground = ground_rotation(p.ground ? p.ground + (long long)inst * 4 : nullptr, Rg);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) sh->M[i * 3 + j] = Rg[i] * Kinv[j] + Rg[3 + i] * Kinv[3 + j] + Rg[6 + i] * Kinv[6 + j];
#pragma unroll
    for (int i = 0; i < 9; ++i) sh->Rg[i] = Rg[i];
  }

#ifdef LA3D_TIMELINE
  // measurement build only (profiles/timeline.py): wall-clock stamps (100 MHz) per workgroup at the phase boundaries,
  // into the workspace behind the launch-order arrays
  double* tl = p.geo + 1024 + (long long)inst * 16;
#define LA3D_STAMP(k) do { if (tid == 0) tl[k] = (double)wall_clock64(); } while (0)
  if (tid == 0) { tl[7] = (double)blockIdx.x; tl[8] = (double)t_entry; sh->tl = tl; }
#else
#define LA3D_STAMP(k) do { } while (0)
#endif
  LA3D_STAMP(0);
  if (!SAMPLE && p.stagger_ticks > 0 && p.order_nch > 0 && blockIdx.x < 1024) {
    // Plain build, u8 planes, size-ordered launch (round 4): the four groups of 256 workgroups that fill the chip start one
    // stagger period apart, the group of the 256 LARGEST instances first (group g of the launch order = blocks [256 g, 256 g + 256)).
    // Every instance streams the same H*W mask bytes whatever its size; started together, the 1024 streams share the bandwidth and
    // nobody's passes begin before ~50 us.  Staggered, the large instances stream at four times the share and are in their (long)
    // passes - VALU work - while the smaller ones, which have the slack, stream.  Measured (helper-kernel build), us per call, without / with 10 us
    // (profiles/r04/r04_stagger.txt): config-2 masks B = 448 / 640 / 1024 / 1280 / 2048: 71.6 / 80.6 / 103.6 / 125.6 / 176.2 ->
    // 66.9 / 74.8 / 99.7 / 118.2 / 170.0; config-5 masks B = 512 / 1024 / 2048: 75.1 / 91.4 / 144.1 -> 69.9 / 83.2 / 139.6; neutral
    // from 4096 up.  Speed only: records do not depend on it.  (Run-length / polygon input has no stream to spread: slower there.)
    const unsigned long long t0 = wall_clock64();
    // (delays 0 / 0.81 / 1.81 / 2.94 periods: the later - smaller - groups wait a little longer each; against equal steps of one
    // period: config 2 at B = 1024 95.1 -> 94.0 us, at 1536 125.6 -> 124.5, config 5 at 1024 equal; equal steps of 10 us are as good on
    // config 2 and 2.7 us worse on config 5 - profiles/r04/r04_stagger.txt, run 5)
    const unsigned g = blockIdx.x >> 8;
    const unsigned long long w = (unsigned long long)p.stagger_ticks * (g == 1 ? 13u : (g == 2 ? 29u : (g == 3 ? 47u : 0u))) / 16u;
    while (wall_clock64() - t0 < w) __builtin_amdgcn_s_sleep(32);
  }
  // reference-subsample mode: this thread's drawn index, requested before the mask stream so that it is not a dependent
  // round trip afterwards (unused when the mask turns out to have <= 500 pixels)
  int my_draw = 0;
  if (SAMPLE && tid < LA3D_NSAMPLE) my_draw = p.sample_idx[(long long)inst * LA3D_NSAMPLE + tid];
  // ---- phase 0: u8 mask plane -> bit image in LDS --------------------------------------
  int nmask = 0;
  if (LDSMASK && RLE) {
    // masks arrive as COCO run lengths: decode straight into the LDS bit image — no u8 plane is ever read
    const long long o0 = p.rle_offsets[inst];
    // (the block totals of the column scan borrow the LDS of the tile list, which is built afterwards)
    nmask = rle_to_bits<NT>(p.rle_counts + o0, (int)(p.rle_offsets[inst + 1] - o0), bits, p.nwords, p.H, p.W, sh->scan, tid,
                            reinterpret_cast<unsigned*>(smem + p_call.mask_lds_bytes + sizeof(Shared)), TILED ? p.list_cap / 2 : 0, p.frame_w);
  } else if (LDSMASK && SRC == 2) {
    // masks arrive as polygon parts (the reference's create_boolean_mask_from_polygon, src/util.py:386-400): rasterised with
    // cv2.fillPoly's rule straight into the LDS bit image; the side stage borrows the space of the tile list
    nmask = poly_to_bits<NT>(p.poly_xy, p.poly_ring_off, p.poly_inst_rings[inst], p.poly_inst_rings[inst + 1],
                             reinterpret_cast<PolySide*>(smem + p_call.mask_lds_bytes + sizeof(Shared)), sh->scan, bits, p.nwords, p.H,
                             p.W, tid, p.frame_w);
  } else if (LDSMASK && SRC == 3) {
    // masks arrive as bit planes: the plane IS the bit image - a straight stream into LDS, no decode (38 400 B for 640x480 against
    // the 307 200 B of a u8 plane)
    // (frames call: the plane lies at its own offset - accepted above, loaded again here -, holds the whole words of the instance's
    // own frame and is 16-byte aligned: always the 16-byte form)
    if constexpr (FRAMES) nmask = bits_plane_to_lds<NT>(p.mask_bits + frame_bits_offset(p_call, inst), bits, p.nwords, HW, 1, tid);
    else nmask = bits_plane_to_lds<NT>(p.mask_bits + (long long)inst * p.bits_plane_stride, bits, p.nwords, HW, p.bits_vec, tid);
  } else if (LDSMASK) {
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
  __syncthreads();
  LA3D_STAMP(1);
  // (from here on the instance index is re-read from LDS: live across the decode stage it costs the polygon build a spilled
  // register pair)
  const int inst_p = __builtin_amdgcn_readfirstlane(sh->order_inst);
  if constexpr (FRAMES) frame_geometry<false, SAMPLE>(p_frame, p_call, p.image_index[inst_p]);   // (re-read for the same reason: see frame_geometry)
  // (and from here on the thread index is rebuilt where it is used - one v_lshl_or from the wave's scalar index and the lane -
  // instead of staying live from kernel entry: with the separable pass in the kernel the allocator otherwise spills it to scratch,
  // and a kernel with scratch launches its waves visibly slower: round 5, B = 8192 590 -> 670 us)
  const int tid_plain = tid;
#define tid (REBUILD_TID ? tid_here(wave, lane) : tid_plain)
  if (SRC != 0 && LDSMASK && p.filter_boundary >= 0) {   // uniform
    // the reference's instance filter (src/util.py:375) on the bit image just built: a dropped instance costs no passes
    int st4[4];
    bits_filter_stats<NT>(bits, p.H, p.frame_w, p.filter_boundary, reinterpret_cast<int*>(sh->part), tid, st4, p.W);   // (frame_w == W unless the rows are padded)
    if (p.filter_stats && tid < 4) (p.filter_stats + (long long)inst_p * 4)[tid] = st4[tid];   // (uniform base: scalar address arithmetic)
    // run lengths: rows holding a pixel (:368-369); polygons: last - first + 1 (:328-335); a bit plane does not say where it came from: the caller's flag
    const int height = SRC == 1 ? st4[1] : (SRC == 3 && !p.bits_span) ? st4[1] : st4[2];
    const bool keep = 16 * height > p.H && st4[3] < p.filter_max_edge && st4[0] >= p.filter_min_area;   // height / H > 0.0625
    if (!keep) {
      if (tid == 0) {
        if (p.aux) {
          double* a = p.aux + (long long)inst_p * LA3D_AUX;
          a[0] = NAN; a[1] = 0.0; a[2] = (double)st4[0]; a[3] = NAN;
        }
        p.status[inst_p] = LA3D_BOX_FILTERED;
        write_nan_box(p.out + (long long)inst_p * LA3D_REC);
        if (p.proj) { for (int j = 0; j < 8; ++j) p.proj[(long long)inst_p * 8 + j] = NAN; }
      }
      return;
    }
  }
  double Mg[9];   // wave-uniform: moved to SGPRs
#pragma unroll
  for (int i = 0; i < 9; ++i) Mg[i] = uniform_f64(sh->M[i]);
  LA3D_STAMP(13);

  // reference-subsample mode: the reference subsamples when in_pc.shape[0] > 500 (src/util_3dbox.py:123) - needs N first.
  // Sampled instances need no tile list (their 500 points are picked through the block prefix, which shares its LDS).
  bool sampled = false;
  int ntot = 0;
  if (SAMPLE) {
    const int wsum = wave_sum_i(nmask);
    if (lane == 0) sh->nmask[wave] = wsum;
    __syncthreads();
    for (int w = 0; w < NWAVE; ++w) ntot += sh->nmask[w];
    // (hull call: every instance goes the sampled way - a mask of <= 500 pixels draws its own ranks 0 .. ntot-1 -, so that its
    // points exist one per thread for the hand-off)
    sampled = HULL || ntot > LA3D_NSAMPLE;
  }

  // ---- active-tile list (deterministic two-pass compaction: count, prefix, write) ----------------
  int nactive = 0, nfull = 0;
  // plain build: the bit image is compacted to the active tiles (eight row words per list entry) and the LDS that frees keeps
  // depth tiles between the passes (sweep_tiled)
  constexpr bool LK = TILED && !SAMPLE;
  int compact = 0;
  // separable single pass (sweep_sep): no ground rotation, no skew - x ray by column, y ray by row, z = depth
  bool sep = false;
  const bool sep_cam = LK && (HULL || !p.sep_off) && Mg[1] == 0.0 && Mg[3] == 0.0 && Mg[6] == 0.0 && Mg[7] == 0.0 && Mg[8] == 1.0;   // uniform
  if (TILED && !sampled) {
    if constexpr (FRAMES) frame_rcp_ntx(p_frame);
    const int ntiles = p.ntx * p.nty, per = p.tiles_per_wave;
    const int tbeg = wave * per, tend = min(tbeg + per, ntiles);
    int base = 0;
    if (per <= 256) {
      // one pass: a wave looks at up to 4 x 64 tiles; the ballots stay in SGPRs across the barrier, the eight row words
      // of a tile are read back to back (rows past the frame re-read the last one), no integer division
      unsigned long long bal[4];
      unsigned wrd[LK ? 4 : 1][8];
      int wcount = 0, fcount = 0;
      unsigned fl = 0;   // bit k: this lane's k-th tile lies completely inside the mask (all eight row words all ones)
      if ((p.H & 7) == 0) {   // uniform: every tile row is complete (the common frame heights) - no row clamp, no select per word
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int t = tbeg + k * 64 + lane;
          unsigned any = 0, all = 0xffffffffu;
          if (t < tend) {
            const int ty = (int)(((float)t + 0.5f) * p.rcp_ntx), tx = t - ty * p.ntx;  // exact: see fit_dispatch
            const unsigned* bw = bits + (ty * 8) * p.ntx + tx;
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
              const unsigned w = bw[rr * p.ntx];
              any |= w;
              if constexpr (LK) { wrd[k][rr] = w; all &= w; }
            }
          }
          bal[k] = __ballot(any != 0);
          wcount += __popcll(bal[k]);
          if constexpr (LK) {
            const bool f = t < tend && all == 0xffffffffu;
            fcount += __popcll(__ballot(f));
            fl |= (f ? 1u : 0u) << k;
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int t = tbeg + k * 64 + lane;
          unsigned any = 0, all = 0xffffffffu;
          if (t < tend) {
            const int ty = (int)(((float)t + 0.5f) * p.rcp_ntx), tx = t - ty * p.ntx;  // exact: see fit_dispatch
            const int rmax = p.H - 1 - ty * 8;                                        // >= 0
            const unsigned* bw = bits + (ty * 8) * p.ntx + tx;
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
              const unsigned w = bw[min(rr, rmax) * p.ntx];
              any |= w;
              if constexpr (LK) { wrd[k][rr] = rr <= rmax ? w : 0u; all &= wrd[k][rr]; }
            }
          }
          bal[k] = __ballot(any != 0);
          wcount += __popcll(bal[k]);
          if constexpr (LK) {
            const bool f = t < tend && all == 0xffffffffu;   // (a tile row past the frame is stored as zeros: never "full")
            fcount += __popcll(__ballot(f));
            fl |= (f ? 1u : 0u) << k;
          }
        }
      }
      if (lane == 0) sh->scan[wave] = (unsigned)wcount | ((unsigned)fcount << 16);   // (at most 256 tiles per wave)
      __syncthreads();
      LA3D_STAMP(14);
      // Round 6: the list holds the tiles that lie completely inside the mask FIRST ([0, nfull): the separable pass walks them with
      // a body that needs no mask bits), the others behind them - each class in tile order.  Any order of the list gives a valid
      // walk; the order only decides how the fp64 partial sums are grouped.
      int fbase = 0;
      for (int w = 0; w < NWAVE; ++w) {
        const int c = (int)(sh->scan[w] & 0xffffu), f = (int)(sh->scan[w] >> 16);
        if (w < wave) { base += c - f; fbase += f; }
        nactive += c;
        nfull += f;
      }
      if (nactive > p.list_cap) {
        nactive = -1;  // uniform: every thread sees the same total
        nfull = 0;
      } else {
        // (with pass-B culling the compact image also holds the survivor list / the depth ranges behind the entries)
        // every wave read its row words before the barrier above: the image region can be overwritten in place
        if constexpr (LK) compact = (nactive * 32 + cull_rng_words(nactive) * 4 <= p.mask_lds_bytes) ? 1 : 0;   // uniform
        int foff = fbase, poff = nfull + base;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool isf = LK && ((fl >> k) & 1u);
          const unsigned long long bf = LK ? __ballot(isf) : 0ull, bp = bal[k] & ~bf, lt = (1ull << lane) - 1ull;
          if ((bal[k] >> lane) & 1ull) {
            const int t = tbeg + k * 64 + lane;
            const int ty = (int)(((float)t + 0.5f) * p.rcp_ntx), tx = t - ty * p.ntx;
            const int idx = isf ? foff + __popcll(bf & lt) : poff + __popcll(bp & lt);
            list[idx] = (unsigned short)((ty << 8) | tx);
            if constexpr (LK) if (compact) {   // uniform
              uint4* e = reinterpret_cast<uint4*>(bits) + 2 * idx;
              e[0] = make_uint4(wrd[k][0], wrd[k][1], wrd[k][2], wrd[k][3]);
              e[1] = make_uint4(wrd[k][4], wrd[k][5], wrd[k][6], wrd[k][7]);
            }
          }
          foff += __popcll(bf); poff += __popcll(bp);
        }
        if constexpr (LK) if (compact) {   // uniform
          if (sep_cam && nactive * 32 + sep_col_words(p.W) * 4 <= p.mask_lds_bytes) {   // uniform
            sep = true;   // per-column depth range behind the entries: [min | max], the identities of unsigned min / max
            unsigned* col = bits + nactive * 8;
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
            nactive += c;
          }
          if (nactive > p.list_cap) { nactive = -1; break; }  // uniform: every thread sees the same total
        }
      }
    }
    LA3D_STAMP(15);
    __syncthreads();
  }

  if constexpr (HULL && LK) {
    // ---- hull call, full-mask mode: the checked separable walk, the axis (the PCA yaw is the fallback), then the hand-off ----
    if (!sep) {   // uniform: no per-column structure (ground rotation, skewed K, too many active tiles) - refused, never fitted as PCA
      if (tid == 0) {
        if (p.aux) {
          double* a = p.aux + (long long)inst_p * LA3D_AUX;
          a[0] = NAN; a[1] = 0.0; a[2] = NAN; a[3] = NAN;
        }
        p.status[inst_p] = LA3D_BOX_UNSUPPORTED;
        write_nan_box(p.out + (long long)inst_p * LA3D_REC);
        if (p.proj) { for (int j = 0; j < 8; ++j) p.proj[(long long)inst_p * 8 + j] = NAN; }
      }
      return;
    }
    unsigned* col = bits + nactive * 8;
    double hacc[5] = {0, 0, 0, 0, 0}, yx[2] = {INFINITY, -INFINITY};
    int hcnt = 0;
    sweep_sep_hull(p, dpl, bits, list, nactive, Mg, col, wave, lane, 0.0, 0.0, hacc, yx, &hcnt, cv);
    stage_moments_to_axis(sh, p, inst_p, hacc, hcnt, nmask, tid, wave, lane, true);
    if (sh->redo) {   // uniform: ill-conditioned raw sums - the moments once more about the pivot the stage left (the ranges stand)
      __syncthreads();
      double piv[2];
      get_pivot(sh, piv);
#pragma unroll
      for (int i = 0; i < 5; ++i) hacc[i] = 0;
      hcnt = 0;
      sweep_sep_hull(p, dpl, bits, list, nactive, Mg, col, wave, lane, piv[0], piv[1], hacc, yx, &hcnt, cv);
      stage_moments_to_axis(sh, p, inst_p, hacc, hcnt, nmask, tid, wave, lane, false);
    }
    if (sh->st != LA3D_BOX_OK) return;   // (the stage wrote status and the NaN record; nothing to finish)
    const double ylo_w = wave_min(yx[0]), yhi_w = wave_max(yx[1]);
    if (lane == 0) { sh->part[wave][5] = ylo_w; sh->part[wave][6] = yhi_w; }
    __syncthreads();
    double* hh = hull_slot(p.geo, inst_p, hull_stride_bytes(false, p.W));
    unsigned* hcol = reinterpret_cast<unsigned*>(hh + HH_D);
    for (int i = tid; i < 2 * p.W; i += NT) hcol[i] = col[i];
    if (tid == 0) {
      double ylo = INFINITY, yhi = -INFINITY;
      for (int w = 0; w < NWAVE; ++w) { ylo = fmin(ylo, sh->part[w][5]); yhi = fmax(yhi, sh->part[w][6]); }
      hh[HH_NVALID] = (double)sh->n_valid; hh[HH_NM] = (double)sh->nm; hh[HH_CYAW] = sh->cyaw; hh[HH_SYAW] = sh->syaw;
      hh[HH_GAP] = sh->gap; hh[HH_YLO] = ylo; hh[HH_YHI] = yhi;
      for (int i = 0; i < 9; ++i) hh[HH_RG + i] = sh->Rg[i];
      hh[HH_A00] = Mg[0]; hh[HH_A02] = Mg[2]; hh[HH_NPTS] = 0.0;
      hh[HH_STATE] = 0.0;
    }
    return;
  }

  // ---- separable single pass: moments, y extent and per-column depth ranges in ONE walk; x / z extents from the ranges -------
  if constexpr (LK) {
    if (sep) {   // uniform
      LA3D_STAMP(2);
      unsigned* col = bits + nactive * 8;
      double sacc[5] = {0, 0, 0, 0, 0}, yx[2] = {INFINITY, -INFINITY};
      unsigned unsafe = 0u;
      if (p.H & 7) sweep_sep<true>(p, dpl, bits, list, nactive, Mg, col, wave, lane, sacc, yx, &unsafe, 0, nfull, cv);   // uniform
      else sweep_sep<false>(p, dpl, bits, list, nactive, Mg, col, wave, lane, sacc, yx, &unsafe, 0, nfull, cv);
      if (__ballot(unsafe >= 0x7f800000u) != 0ull && lane == 0) sh->sep_bad = 1;   // NaN / inf / negative depth under the mask
      // (the wave's y extent waits in scalar registers while the axis is computed: four vector registers fewer across that stage)
      const double ylo_w = uniform_f64(wave_min(yx[0])), yhi_w = uniform_f64(wave_max(yx[1]));
      LA3D_STAMP(3);
      stage_moments_to_axis(sh, p, inst_p, sacc, nmask, nmask, tid, wave, lane, true);
      LA3D_STAMP(4);
      if (!(sh->redo || sh->sep_bad)) {   // uniform
        if (sh->st != LA3D_BOX_OK) return;
        double N0[3], N2[3], ext[6];
        yaw_rows(sh, Mg, N0, N2);
        sep_col_extents(col, p.W, N0, N2, tid, ext);
        ext[2] = ylo_w; ext[3] = yhi_w;
        LA3D_STAMP(5);
        if constexpr (FRAMES) frame_proj(p_frame, p_call, inst_p);
        stage_extents_to_box(sh, p, inst_p, ext, tid, wave, lane);
        stage_status_aux(sh, p, inst_p, tid);
        LA3D_STAMP(6);
        return;
      }
      __syncthreads();   // everyone has read redo / sep_bad and the partials: on to the general two-pass path
    }
  }

  // pass-B tile culling (see cull_plan): instances with enough active tiles record every tile's depth range in pass A
  bool cull = false;
  int rng_words = 0;
  if constexpr (LK) {
    // (every compact instance reserves the area: pass B always walks a survivor list - the identity when nothing is culled)
    if (compact) {   // uniform
      rng_words = cull_rng_words(nactive);
      cull = nactive >= p.cull_min && nactive <= CULL_MAXT;
      if (!cull) {
        unsigned short* surv = reinterpret_cast<unsigned short*>(bits + nactive * 8);
        // (vectorised, the index vector tid + {0, 512, 1024, 1536} becomes a 128-bit register tuple that lives from kernel entry: a spill)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (int t = tid; t < nactive; t += NT) surv[t] = (unsigned short)t;   // (visible after the barriers of the axis stage)
      }
    }
  }

  LA3D_STAMP(2);
  // ---- pass A: moments ------------------------------------------------------------------
  double acc[5] = {0, 0, 0, 0, 0};
  int cnt = 0;
  // sampled-point state (SAMPLE only): the point of this thread in the ground-aligned frame
  double px = 0, py = 0, pz = 0;
  bool pok = false;

  if (SAMPLE) {
    if (sampled) {
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
        int r = (HULL && ntot <= LA3D_NSAMPLE) ? tid_plain : my_draw;
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
        if constexpr (FRAMES) p_frame.rcpW = 1.0f / (float)p.W;
        pix_uv(i, p.W, p.rcpW, &u, &v);
        const double ud = (double)u, vd = (double)v;
        pok = finite_f32(df);
        const double d = pok ? (double)df : 0.0;
        px = d * fma(Mg[0], ud, fma(Mg[1], vd, Mg[2]));
        py = d * fma(Mg[3], ud, fma(Mg[4], vd, Mg[5]));
        pz = d * fma(Mg[6], ud, fma(Mg[7], vd, Mg[8]));
        if (pok) {
          acc[0] = px; acc[1] = pz; acc[2] = px * px; acc[3] = px * pz; acc[4] = pz * pz;
          cnt = 1;
        }
      }
    }
  }
  // TILED: optimistic pass first (no per-pixel finite test); a non-finite masked depth shows up as non-finite sums and
  // the workgroup falls back to the checked passes.  Same records either way.
  bool checked = !TILED;
  if (!sampled) {
    if (TILED) {
      // (the un-grounded, skew-free forms of the pixel math where they apply: same records, fewer instructions - quad_math)
      // (not in the subsample build, which walks tiles only for its small masks and has no registers to spare)
      constexpr bool SP = !SAMPLE;
      const bool specA = SP && Mg[6] == 0.0 && Mg[7] == 0.0 && Mg[8] == 1.0;   // uniform
      if (LK && cull) {
        if (specA) sweep_tiled<0, false, true, SP>(p, dpl, bits, list, nactive, Mg, Mg + 3, Mg + 6, wave, lane, acc, &cnt, nullptr, compact, rng_words, -1, nfull, cv);
        else sweep_tiled<0, false, true>(p, dpl, bits, list, nactive, Mg, Mg + 3, Mg + 6, wave, lane, acc, &cnt, nullptr, compact, rng_words, -1, nfull, cv);
      } else {
        if (specA) sweep_tiled<0, false, false, SP>(p, dpl, bits, list, nactive, Mg, Mg + 3, Mg + 6, wave, lane, acc, &cnt, nullptr, compact, rng_words, -1, nfull, cv);
        else sweep_tiled<0, false>(p, dpl, bits, list, nactive, Mg, Mg + 3, Mg + 6, wave, lane, acc, &cnt, nullptr, compact, rng_words, -1, nfull, cv);
      }
      cnt = nmask;   // the optimistic pass does not count: with every masked depth finite, valid pixels = mask pixels
    }
    else sweep<VEC, LDSMASK, 0>(p, dpl, mpl, bits, Mg, Mg + 3, Mg + 6, wave, lane, acc, &cnt, &nmask, nullptr, cv);
  }

  LA3D_STAMP(3);
  stage_moments_to_axis(sh, p, inst_p, acc, cnt, nmask, tid, wave, lane, true);
  if (sh->redo) {  // uniform: non-finite sums (the optimistic tiled pass) or ill-conditioned ones (axis_from_sums) - the checked pass
                   // about the pivot the stage left (zero unless the sums were ill-conditioned)
    __syncthreads();        // everyone has read sh->redo and the partials before they are rewritten (the pivot stays where it is)
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i] = 0;
    cnt = 0;
    if (sampled) {
      if (pok) {
        const double x = px - pivot_ptr(sh)[0], z = pz - pivot_ptr(sh)[1];
        acc[0] = x; acc[1] = z; acc[2] = x * x; acc[3] = x * z; acc[4] = z * z;
        cnt = 1;
      }
    } else if (TILED) {
      if (sh->redo == 2) {   // ill-conditioned sums: the moments about the pivot; the optimistic pass's tile ranges and pass B stand
        pivot_pass(p, dpl, bits, list, nactive, Mg, Mg + 6, wave, lane, compact, pivot_ptr(sh), acc, &cnt, cv);
      } else {
        checked = true;
        if (LK && cull) sweep_tiled<0, true, true>(p, dpl, bits, list, nactive, Mg, Mg + 3, Mg + 6, wave, lane, acc, &cnt, nullptr, compact, rng_words, -1, nfull, cv);
        else sweep_tiled<0, true>(p, dpl, bits, list, nactive, Mg, Mg + 3, Mg + 6, wave, lane, acc, &cnt, nullptr, compact, rng_words, -1, nfull, cv);
      }
    } else {
      double piv[2];
      get_pivot(sh, piv);
      sweep<VEC, LDSMASK, 0, true>(p, dpl, mpl, bits, Mg, Mg + 3, Mg + 6, wave, lane, acc, &cnt, &nmask, piv, cv);
    }
    stage_moments_to_axis(sh, p, inst_p, acc, cnt, nmask, tid, wave, lane, false);
  }
  LA3D_STAMP(4);
  if (sh->st != LA3D_BOX_OK) return;

  if constexpr (HULL && SAMPLE) {
    // ---- hull call, reference-subsample mode: the at most 500 points in the ground-aligned frame, one per thread, handed over ----
    double* hh = hull_slot(p.geo, inst_p, hull_stride_bytes(true, p.W));
    if (tid_plain < HULL_SMALL) {
      double* q = hh + HH_D + 3 * tid_plain;
      q[0] = pok ? px : NAN; q[1] = pok ? py : NAN; q[2] = pok ? pz : NAN;
    }
    if (tid_plain == 0) {
      hh[HH_NVALID] = (double)sh->n_valid; hh[HH_NM] = (double)sh->nm; hh[HH_CYAW] = sh->cyaw; hh[HH_SYAW] = sh->syaw;
      hh[HH_GAP] = sh->gap; hh[HH_YLO] = 0.0; hh[HH_YHI] = 0.0;
      for (int i = 0; i < 9; ++i) hh[HH_RG + i] = sh->Rg[i];
      hh[HH_A00] = 0.0; hh[HH_A02] = 0.0; hh[HH_NPTS] = (double)min(ntot, LA3D_NSAMPLE);
      hh[HH_STATE] = 0.0;
    }
    return;
  }

  // ---- pass B: extents along the principal axes -----------------------------------------
  double ext[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};  // x, y, z : lo, hi
  if (sampled) {
    if (pok) {  // exactly the reference's arithmetic: rotate_y(yaw) applied to the stored point
      const double x2 = sh->cyaw * px + sh->syaw * pz;
      const double z2 = -sh->syaw * px + sh->cyaw * pz;
      ext[0] = ext[1] = x2;
      ext[2] = ext[3] = py;
      ext[4] = ext[5] = z2;
    }
  } else {
    double N0[3], N2[3];
    yaw_rows(sh, Mg, N0, N2);
    int d0 = 0, d1 = 0;
    if (TILED) {
      // (pass B pulls its tiles from an LDS work queue: run-length input 74.8 -> 71.3 us, B = 512 88.7 -> 85.5, config 5 at 16 k
      // 945 -> 927; profiles/r03/r03_pass_b_queue.txt)
      unsigned* qh = &sh->qhead;
      int nsurv = -1;
      if constexpr (LK) {
        if (compact) nsurv = nactive;   // the identity list written before the axis stage
        if (cull) {   // uniform
          nsurv = checked ? cull_plan<true>(sh, p, dpl, bits, list, nactive, rng_words, N0, Mg + 3, N2, tid, wave, lane, ext, cv)
                          : cull_plan<false>(sh, p, dpl, bits, list, nactive, rng_words, N0, Mg + 3, N2, tid, wave, lane, ext, cv);
        }
      }
      if (checked) sweep_tiled<1, true>(p, dpl, bits, list, nactive, N0, Mg + 3, N2, wave, lane, ext, &d0, qh, compact, rng_words, nsurv, 0, cv);
      else if (!SAMPLE && Mg[3] == 0.0) sweep_tiled<1, false, false, !SAMPLE>(p, dpl, bits, list, nactive, N0, Mg + 3, N2, wave, lane, ext, &d0, qh, compact, rng_words, nsurv, 0, cv);
      else sweep_tiled<1, false>(p, dpl, bits, list, nactive, N0, Mg + 3, N2, wave, lane, ext, &d0, qh, compact, rng_words, nsurv, 0, cv);
    }
    else sweep<VEC, LDSMASK, 1>(p, dpl, mpl, bits, N0, Mg + 3, N2, wave, lane, ext, &d0, &d1, nullptr, cv);
  }
  LA3D_STAMP(5);
  if constexpr (FRAMES) frame_proj(p_frame, p_call, inst_p);
  stage_extents_to_box(sh, p, inst_p, ext, tid, wave, lane);
  stage_status_aux(sh, p, inst_p, tid);
  LA3D_STAMP(6);
}
#undef tid



#if LA3D_INSTANCE_DT == 0   // (the kernels behind the fit - they read no depth - exist once: the 16-bit units launch them through hull_finish_launch / hull_refuse_launch)
// ------------------------------------------------------------------------------------------
// hull finish: one workgroup of NTP threads per instance - candidates -> hull_yaw -> extents over the candidates under the hull yaw
// (the extents of a point set along ANY direction are taken at hull vertices, and every hull vertex is a candidate) -> record.
// ------------------------------------------------------------------------------------------
struct alignas(16) SharedF {
  double part[NWAVEP][8];
  double cyaw, syaw;
  int nvalid;       // candidates held in hs.x / hs.z (hull_yaw's point count)
  int hull_n;
  int fill;
};

template <bool SAMPLE, int HCAP>
__global__ __launch_bounds__(NTP) void hull_finish_kernel(const FitParams p, unsigned long long stride) {
  __shared__ SharedF sh;
  __shared__ SharedHullT<HCAP> hs;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int inst = blockIdx.x;
  const double* hh = hull_slot(p.geo, inst, (size_t)stride);
  if (hh[HH_STATE] != 0.0) return;   // uniform: the fit kernel has finished this instance itself
  if (tid == 0) { sh.fill = 0; sh.hull_n = 0; }
  __syncthreads();
  double ylo = INFINITY, yhi = -INFINITY;
  if (SAMPLE) {
    const int npts = min((int)hh[HH_NPTS], HULL_SMALL);
    const double* pts = hh + HH_D;
    for (int i = tid; i < npts; i += NTP) {
      const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
      if (x == x) {   // (a point the fit kernel dropped is three NaNs)
        const int slot = atomicAdd(&sh.fill, 1);
        if (slot < HCAP) { hs.x[slot] = x; hs.z[slot] = z; }
        ylo = fmin(ylo, y); yhi = fmax(yhi, y);
      }
    }
  } else {
    const unsigned* col = reinterpret_cast<const unsigned*>(hh + HH_D);
    const double a00 = hh[HH_A00], a02 = hh[HH_A02];
    if (tid == 0) { ylo = hh[HH_YLO]; yhi = hh[HH_YHI]; }
    for (int u = tid; u < p.W; u += NTP) {
      const unsigned lo = col[u], hi = col[p.W + u];
      if (lo <= hi) {   // the column holds a valid pixel: the two ends of its ray (one point when they coincide)
        const int k = lo == hi ? 1 : 2;
        const int slot = atomicAdd(&sh.fill, k);
        if (slot + k <= HCAP) {
          const double r0 = fma(a00, (double)u, a02), dlo = (double)hull_unkey(lo), dhi = (double)hull_unkey(hi);
          hs.x[slot] = dlo * r0; hs.z[slot] = dlo;
          if (k == 2) { hs.x[slot + 1] = dhi * r0; hs.z[slot + 1] = dhi; }
        }
      }
    }
  }
  __syncthreads();
  const int n = sh.fill;
  double* out = p.out + (long long)inst * LA3D_REC;
  double* aux = p.aux ? p.aux + (long long)inst * LA3D_AUX : nullptr;
  if (n > HCAP) {   // uniform: more than HCAP candidates (one per column whose two ends coincide, two otherwise) - refused, never fitted as PCA
    if (tid == 0) {
      if (aux) { aux[0] = NAN; aux[1] = hh[HH_NVALID]; aux[2] = hh[HH_NM]; aux[3] = NAN; }
      p.status[inst] = LA3D_BOX_UNSUPPORTED;
      write_nan_box(out);
      if (p.proj) { for (int j = 0; j < 8; ++j) p.proj[(long long)inst * 8 + j] = NAN; }
    }
    return;
  }
  if (tid == 0) { sh.nvalid = n; sh.cyaw = hh[HH_CYAW]; sh.syaw = hh[HH_SYAW]; }
  __syncthreads();
  double yaw = 0.0;
  const bool by_hull = hull_yaw(&hs, &sh, tid, &yaw);   // false: fewer than 3 hull vertices - the PCA axis stands (reference :222-224)
  if (by_hull && tid == 0) {
    double s_, c_;
    sincos(yaw, &s_, &c_);
    sh.cyaw = c_; sh.syaw = s_;
  }
  __syncthreads();
  const double cy = sh.cyaw, sy = sh.syaw;
  double xlo = INFINITY, xhi = -INFINITY, zlo = INFINITY, zhi = -INFINITY;
  for (int i = tid; i < n; i += NTP) {
    const double x = hs.x[i], z = hs.z[i];
    const double x2 = cy * x + sy * z, z2 = -sy * x + cy * z;   // rotate_y(yaw) @ rotated^T  (:154)
    xlo = fmin(xlo, x2); xhi = fmax(xhi, x2); zlo = fmin(zlo, z2); zhi = fmax(zhi, z2);
  }
  {
    const double r0 = wave_min(xlo), r1 = wave_max(xhi), r2 = wave_min(zlo), r3 = wave_max(zhi), r4 = wave_min(ylo), r5 = wave_max(yhi);
    if (lane == 0) { double* pp = sh.part[wave]; pp[0] = r0; pp[1] = r1; pp[2] = r2; pp[3] = r3; pp[4] = r4; pp[5] = r5; }
  }
  __syncthreads();
  if (wave == 0) {
    double xmin = INFINITY, xmax = -INFINITY, zmin = INFINITY, zmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int w = 0; w < NWAVEP; ++w) {
      xmin = fmin(xmin, sh.part[w][0]); xmax = fmax(xmax, sh.part[w][1]); zmin = fmin(zmin, sh.part[w][2]); zmax = fmax(zmax, sh.part[w][3]);
      ymin = fmin(ymin, sh.part[w][4]); ymax = fmax(ymax, sh.part[w][5]);
    }
    double Rg[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rg[i] = hh[HH_RG + i];
    if (p.proj) {   // uniform
      const int img = p.image_index ? p.image_index[inst] : inst;
      write_box_wave(out, Rg, cy, sy, xmin, xmax, ymin, ymax, zmin, zmax, lane, p.proj + (long long)inst * 8, p.K + (long long)img * p.k_stride,
                     p.proj_w, p.proj_h);
    } else {
      write_box_wave(out, Rg, cy, sy, xmin, xmax, ymin, ymax, zmin, zmax, lane);
    }
  } else if (tid == 64) {
    if (aux) {
      aux[0] = by_hull ? yaw : atan2(sy, cy); aux[1] = hh[HH_NVALID]; aux[2] = hh[HH_NM];
      aux[3] = by_hull ? -(double)sh.hull_n : hh[HH_GAP];   // negative: the hull decided the yaw (value = number of hull vertices)
    }
    p.status[inst] = LA3D_BOX_OK;
  }
}

// a hull call in full-mask mode on a frame outside the tiled vector path: every instance is refused (status 5, NaN record)
__global__ __launch_bounds__(256) void hull_refuse_kernel(const FitParams p) {
  const int inst = blockIdx.x * 256 + threadIdx.x;
  if (inst >= p.B) return;
  if (p.aux) { double* a = p.aux + (long long)inst * LA3D_AUX; a[0] = NAN; a[1] = 0.0; a[2] = NAN; a[3] = NAN; }
  p.status[inst] = LA3D_BOX_UNSUPPORTED;
  write_nan_box(p.out + (long long)inst * LA3D_REC);
  if (p.proj) { for (int j = 0; j < 8; ++j) p.proj[(long long)inst * 8 + j] = NAN; }
}

#endif   // LA3D_INSTANCE_DT == 0

// the two launches of a hull call, one linear chain on the caller's stream (no launch order: workgroup b fits instance xcd_remap(b))
template <bool VEC, bool SAMPLE, int SRC>
int launch_hull_inst(const KParams& p, size_t lds, hipStream_t s) {
  // (full-mask mode = the tiled vector build, subsample mode = the build without tile list)
  auto kern = fit_instances_kernel<VEC, true, SAMPLE, !SAMPLE, SRC, true>;
  allow_big_lds(reinterpret_cast<const void*>(kern));
  hipLaunchKernelGGL(kern, dim3(p.B), dim3(NT), lds, s, p);
  const int rc = check_launch("fit_instances_kernel (hull)");
  if (rc != LA3D_SUCCESS) return rc;
  return la3d::hull_finish_launch(p, SAMPLE, s);
}
template <bool VEC, bool SAMPLE>
int launch_hull(const KParams& p, size_t lds, hipStream_t s) {
  if (p.mask_bits != nullptr) return launch_hull_inst<true, SAMPLE, 3>(p, lds, s);
  if (p.rle_counts != nullptr) return launch_hull_inst<true, SAMPLE, 1>(p, lds, s);
  if (p.poly_xy != nullptr) return launch_hull_inst<true, SAMPLE, 2>(p, lds, s);
  return launch_hull_inst<VEC, SAMPLE, 0>(p, lds, s);
}

template <bool VEC, bool LDSMASK, bool SAMPLE, bool TILED, int SRC, bool FRAMES = false>
int launch_fit_inst(const KParams& p_in, size_t lds, hipStream_t s, void* workspace) {
  auto kern = fit_instances_kernel<VEC, LDSMASK, SAMPLE, TILED, SRC, false, FRAMES>;
  allow_big_lds(reinterpret_cast<const void*>(kern));
  KParams p = p_in;
  // size-balanced launch order: needs the 16-byte mask groups (VEC), more than one workgroup per CU, and a batch
  // the O(B^2) ranking is cheap for
  // (a frames call orders by the caller's area_hint only: the estimates know one frame size per call)
  if (workspace && VEC && !SAMPLE && p.B > 256 && p.B <= ORDER_MAX_B && balance_enabled(p) && (!FRAMES || p.area_hint)) {
    int wg_per_cu = 2048 / NT;  // wave slots: 32 per CU at 64 VGPRs
    const int by_lds = (int)((160 * 1024) / (lds ? lds : 1));
    if (by_lds < wg_per_cu) wg_per_cu = by_lds;
    if (wg_per_cu >= 1 && p.B <= BALANCE_MAX_ROUNDS * wg_per_cu * 256) {
      p.order_nch = (p.B + ORDER_CHUNK - 1) / ORDER_CHUNK;
      p.order_resident = wg_per_cu * 256;
      const OrderKeyScale k = order_key_scale(p);
      if (p.area_hint) {   // the caller knows the mask areas (annotation metadata, a preceding filter): no helper launch at all
        p.order_shift = k.shift;
      } else {
        unsigned* est = static_cast<unsigned*>(workspace);  // [B] sort keys
        p.order_keys = est;
        bool self = config().order_self != 0 && wg_per_cu * 256 >= 256;
#ifdef LA3D_TIMELINE
        self = false;   // (the stamp rows of the measurement build live where the nonces would)
#endif
        // a call captured into a HIP graph would replay with the SAME nonce: the records of the previous replay would read as
        // complete while this replay's keys are still on their way - with new masks in the same buffers, two workgroups could rank
        // with different keys.  Captured calls keep the helper kernel.
        if (self && stream_capturing(s)) self = false;
        if (self) {
          // no helper launch: the fit kernel estimates in its prologue (estimate_publish); nonces behind the keys, 256-byte aligned
          p.order_self = config().order_self; p.est_step = k.step; p.order_shift = k.shift;
          p.order_flags = reinterpret_cast<unsigned long long*>(static_cast<unsigned char*>(workspace) + (((size_t)p.B * 4 + 255) & ~(size_t)255));
          const unsigned long long t = (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count();
          p.order_nonce = (t * 0x9E3779B97F4A7C15ull) ^ (unsigned long long)reinterpret_cast<uintptr_t>(workspace) ^ 0xA5A5A5A55A5A5A5Aull;
        } else if (SRC == 3) {
          hipLaunchKernelGGL(size_estimate_bits_kernel, dim3((p.B + 3) / 4), dim3(256), 0, s, static_cast<const FitParams&>(p), k.shift, est);
        } else {
          hipLaunchKernelGGL(size_estimate_kernel, dim3((p.B + 3) / 4), dim3(256), 0, s, p.mask, p.rle_counts, p.rle_offsets, p.poly_xy,
                             p.poly_ring_off, p.poly_inst_rings, p.B, p.HW, k.step, k.shift, est, nullptr);
        }
      }
    }
  }
  hipLaunchKernelGGL(kern, dim3(p.B), dim3(NT), lds, s, p);
  return check_launch("fit_instances_kernel");
}


// run-length input is its own instantiation (it needs the LDS bit image), so the u8 kernels carry no decode code
template <bool VEC, bool LDSMASK, bool SAMPLE, bool TILED = false>
int launch_fit(const KParams& p, size_t lds, hipStream_t s, void* workspace = nullptr) {
  if (LDSMASK && p.mask_bits != nullptr) return launch_fit_inst<VEC, LDSMASK, SAMPLE, TILED, LDSMASK ? 3 : 0>(p, lds, s, workspace);
  if (LDSMASK && p.rle_counts != nullptr) return launch_fit_inst<VEC, LDSMASK, SAMPLE, TILED, LDSMASK ? 1 : 0>(p, lds, s, workspace);
  if (LDSMASK && p.poly_xy != nullptr) return launch_fit_inst<VEC, LDSMASK, SAMPLE, TILED, LDSMASK ? 2 : 0>(p, lds, s, workspace);
  return launch_fit_inst<VEC, LDSMASK, SAMPLE, TILED, 0>(p, lds, s, workspace);
}


// la3d_fit_instances_frames / la3d_fit_instances_frames_depth16: run lengths or polygon parts, la3d_fit_instances_frames_bits: bit
// planes - the tiled form (full-mask or subsample)
template <bool SAMPLE>
int launch_fit_frames(const KParams& p, size_t lds, hipStream_t s, void* workspace) {
  if (p.mask_bits != nullptr) return launch_fit_inst<true, true, SAMPLE, true, 3, true>(p, lds, s, workspace);
  if (p.rle_counts != nullptr) return launch_fit_inst<true, true, SAMPLE, true, 1, true>(p, lds, s, workspace);
  return launch_fit_inst<true, true, SAMPLE, true, 2, true>(p, lds, s, workspace);
}

}  // namespace

namespace la3d {
#if LA3D_INSTANCE_DT == 0
int hull_finish_launch(const FitParams& p, bool sample, hipStream_t s) {
  const unsigned long long stride = hull_stride_bytes(sample, p.W);
  if (sample) hipLaunchKernelGGL((hull_finish_kernel<true, HULL_SMALL>), dim3(p.B), dim3(NTP), 0, s, p, stride);
  else hipLaunchKernelGGL((hull_finish_kernel<false, HULL_MAX>), dim3(p.B), dim3(NTP), 0, s, p, stride);
  return check_launch("hull_finish_kernel");
}
int hull_refuse_launch(const FitParams& p, hipStream_t s) {
  hipLaunchKernelGGL(hull_refuse_kernel, dim3((p.B + 255) / 256), dim3(256), 0, s, p);
  return check_launch("hull_refuse_kernel");
}
#endif

int LA3D_INSTANCE_FIT(KParams p, const CallFacts& f, hipStream_t s, void* workspace, const char* who) {
  const int H = p.H, W = p.W, B = p.B;
  const bool vec = f.vec, ldsmask = f.ldsmask;
  const size_t poly_stage = f.poly_stage;
  size_t lds = f.lds;
  const unsigned char* mask = p.mask;
  if (f.sample) {
    if (!ldsmask) {
      snprintf(g_err, sizeof(g_err), "%s: reference-subsample mode needs the bit image in LDS (H*W <= 1048576)", who);
      return LA3D_ERR_UNSUPPORTED;
    }
    const size_t blocks = (size_t)rank_prefix_bytes(p.nwords);   // one prefix word per 32-word block of the bit image
    lds += blocks > poly_stage ? blocks : poly_stage;
    if (lds > 160 * 1024 - 256) {
      snprintf(g_err, sizeof(g_err), "%s: reference-subsample mode: frame too large for LDS", who);
      return LA3D_ERR_UNSUPPORTED;
    }
    if (f.method == LA3D_METHOD_CONVEX_HULL) {   // every instance goes the sampled way: no tile list
      p.geo = static_cast<double*>(f.hull_area);
      return vec ? launch_hull<true, true>(p, lds, s) : launch_hull<false, true>(p, lds, s);
    }
    if (vec && W % 32 == 0 && W / 32 <= 255 && (H + 7) / 8 <= 255) {
      // masks of <= 500 px (not sampled) walk their active tiles; the list shares the LDS of the block prefix
      p.ntx = W / 32; p.nty = (H + 7) / 8;
      p.rcp_ntx = 1.0f / (float)p.ntx;
      p.tiles_per_wave = (p.ntx * p.nty + NWAVE - 1) / NWAVE;
      const size_t fixed = lds - (blocks > poly_stage ? blocks : poly_stage);
      int budget = 0;                                          // four workgroups per CU if the frame allows (tiled_list_cap)
      const long cap = tiled_list_cap<true>(p.mask_lds_bytes, p.nwords, p.ntx * p.nty, &budget);
      if (cap >= 64 && budget <= 160 * 1024 - 256) {
        p.list_cap = (int)cap;
        const size_t tail = (size_t)cap * 2 > blocks ? (size_t)cap * 2 : blocks;
        if (f.frames) return launch_fit_frames<true>(p, fixed + (tail > poly_stage ? tail : poly_stage), s, nullptr);
        return launch_fit<true, true, true, true>(p, fixed + (tail > poly_stage ? tail : poly_stage), s);
      }
    }
    if (f.frames) {
      snprintf(g_err, sizeof(g_err), "%s: reference-subsample mode: bounds outside the tiled form: H <= 2040, W <= 8160, and bit image + rank "
               "prefix + 64 tile-list entries within one workgroup's LDS (160 KiB)", who);
      return LA3D_ERR_UNSUPPORTED;
    }
    return vec ? launch_fit<true, true, true>(p, lds, s) : launch_fit<false, true, true>(p, lds, s);
  }
  // tiled fast path: 32-px-wide tiles map to exactly one bit-image word / one 128-B depth line per row
  p.ntx = W / 32; p.nty = (H + 7) / 8;
  // ty = int((t + 0.5f) * rcp_ntx) is exact for t < 65536: the fraction of (t+0.5)/ntx stays at least 0.5/ntx away from
  // an integer and the float error is below (65536/ntx) * 1.2e-7
  p.rcp_ntx = 1.0f / (float)(p.ntx > 0 ? p.ntx : 1);
  p.tiles_per_wave = (p.ntx * p.nty + NWAVE - 1) / NWAVE;
  if (ldsmask && vec && W % 32 == 0 && p.ntx <= 255 && p.nty <= 255) {
    // LDS per workgroup: the largest number of workgroups per CU (160 KiB LDS) that still leaves room
    // for a useful list (tiled_list_cap); masks with more active tiles than the cap take the dense walk
    const size_t fixed = lds;
    const long cap = tiled_list_cap<false>(p.mask_lds_bytes, p.nwords, p.ntx * p.nty);
    if (cap >= 64) {
      p.list_cap = (int)cap;
      if (f.method == LA3D_METHOD_CONVEX_HULL) {
        p.geo = static_cast<double*>(f.hull_area);
        return launch_hull<true, false>(p, fixed + ((size_t)cap * 2 > poly_stage ? (size_t)cap * 2 : poly_stage), s);
      }
      if (f.frames) return launch_fit_frames<false>(p, fixed + ((size_t)cap * 2 > poly_stage ? (size_t)cap * 2 : poly_stage), s, workspace);
      if (mask != nullptr && B > 256) {
        // u8 planes: the resident groups start one group's stream time apart - 256 x H*W bytes at the ~6.4 TB/s a pure reader gets:
        // 12.3 us for 640x480 (the kernel applies it only under the size-ordered launch; LA3D_STAGGER_US overrides, 0 switches it
        // off).  Measured with the self-estimating launch (profiles/r04/r04_stagger.txt, run 4), us per call at 6 / 8 / 10 / 12 / 14 us:
        // config-2 masks B = 1024: 96.0 / 94.8 / 93.4 / 94.5 / 95.4, B = 1536: 130.4 / 127.4 / 124.9 / 125.0 / 124.3; config-5 masks
        // B = 1024: 84.8 / 82.5 / 80.4 / 78.1 / 77.5 - the config-2 optimum is 10, the skewed mix wants more: one stream time is between.
        double us = 256.0 * (double)p.HW / 6.4e6;
        if (config().stagger_us >= 0) us = config().stagger_us;
        p.stagger_ticks = (int)(us * 100.0);
      }
      return launch_fit<true, true, false, true>(p, fixed + ((size_t)cap * 2 > poly_stage ? (size_t)cap * 2 : poly_stage), s, workspace);
    }
  }
  if (f.frames) {
    snprintf(g_err, sizeof(g_err), "%s: bounds outside the tiled form: H <= 2040, W <= 8160, and bit image + 64 tile-list entries within one "
             "workgroup's LDS (160 KiB)", who);
    return LA3D_ERR_UNSUPPORTED;
  }
  if (f.method == LA3D_METHOD_CONVEX_HULL) {
    // full-mask hull on a frame outside the tiled vector path: no per-column structure to take the hull from - every instance is
    // refused (LA3D_BOX_UNSUPPORTED); reference-subsample mode (sample_idx) covers such frames
    return hull_refuse_launch(p, s);
  }
  lds += poly_stage;
  if (ldsmask) return vec ? launch_fit<true, true, false>(p, lds, s, workspace) : launch_fit<false, true, false>(p, lds, s);
  return vec ? launch_fit<true, false, false>(p, lds, s) : launch_fit<false, false, false>(p, lds, s);
}
}  // namespace la3d
