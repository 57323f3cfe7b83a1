// la3d_instance.hip - the INSTANCE ENGINE of la3d_fit_instances: one 512-thread workgroup per instance (mask -> bit image in LDS ->
// active-tile list -> separable single pass, or pass A / axis / pass B -> record), its launch order helper kernel and its launcher.
// Design and measurements: DESIGN.md section 4.1; the walks and stages it is built from: la3d_walks.hpp, la3d_stages.hpp.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "la3d_device.hpp"
#include "la3d_poly.hpp"
#include "la3d_engines.hpp"
#include "la3d_walks.hpp"
#include "la3d_stages.hpp"
#include "la3d_instance_phases.hpp"
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
  return uniform_i64(off_v);
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

// ---- hull call, full-mask mode: the checked separable walk, the axis (the PCA yaw is the fallback), then the hand-off of
// hull_finish_kernel - the per-column depth ranges and the header.  (The thread index is rebuilt at each use: see the kernel.) ----
__device__ inline void hull_full_mask(Shared* sh, const FitParams& p, int inst, const DepthT* __restrict__ dpl, unsigned* bits, const unsigned short* list,
                                      int nactive, bool sep, const double* Mg, int nmask, int wave, int lane, const DepthCvt<DepthT> cv) {
  if (!sep) {   // uniform: no per-column structure (ground rotation, skewed K, too many active tiles) - refused, never fitted as PCA
    if (tid_here(wave, lane) == 0) write_no_box(p, inst, LA3D_BOX_UNSUPPORTED, 0.0, NAN);
    return;
  }
  unsigned* col = bits + nactive * 8;
  double hacc[5] = {0, 0, 0, 0, 0}, yx[2] = {INFINITY, -INFINITY};
  int hcnt = 0;
  sweep_sep_hull(p, dpl, bits, list, nactive, Mg, col, wave, lane, 0.0, 0.0, hacc, yx, &hcnt, cv);
  stage_moments_to_axis(sh, p, inst, hacc, hcnt, nmask, tid_here(wave, lane), wave, lane, true);
  if (sh->redo) {   // uniform: ill-conditioned raw sums - the moments once more about the pivot the stage left (the ranges stand)
    __syncthreads();
    double piv[2];
    get_pivot(sh, piv);
#pragma unroll
    for (int i = 0; i < 5; ++i) hacc[i] = 0;
    hcnt = 0;
    sweep_sep_hull(p, dpl, bits, list, nactive, Mg, col, wave, lane, piv[0], piv[1], hacc, yx, &hcnt, cv);
    stage_moments_to_axis(sh, p, inst, hacc, hcnt, nmask, tid_here(wave, lane), wave, lane, false);
  }
  if (sh->st != LA3D_BOX_OK) return;   // (the stage wrote status and the NaN record; nothing to finish)
  const double ylo_w = wave_min(yx[0]), yhi_w = wave_max(yx[1]);
  if (lane == 0) { sh->part[wave][5] = ylo_w; sh->part[wave][6] = yhi_w; }
  __syncthreads();
  double* hh = hull_slot(p.geo, inst, hull_stride_bytes(false, p.W));
  unsigned* hcol = reinterpret_cast<unsigned*>(hh + HH_D);
  for (int i = tid_here(wave, lane); i < 2 * p.W; i += NT) hcol[i] = col[i];
  if (tid_here(wave, lane) == 0) {
    double ylo = INFINITY, yhi = -INFINITY;
    for (int w = 0; w < NWAVE; ++w) { ylo = fmin(ylo, sh->part[w][5]); yhi = fmax(yhi, sh->part[w][6]); }
    hull_handoff_header(hh, sh, ylo, yhi, Mg[0], Mg[2], 0.0);
  }
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
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* bits = reinterpret_cast<unsigned*>(smem);
  Shared* sh = reinterpret_cast<Shared*>(smem + p_call.mask_lds_bytes);
  unsigned* prefix = reinterpret_cast<unsigned*>(smem + p_call.mask_lds_bytes + sizeof(Shared));  // SAMPLE only
  // TILED only: compacted list of active tile ids (before it is built, the mask decoders borrow its LDS: mask_to_bits)
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
      // before anything is read through it (no barrier has been passed: the whole workgroup leaves)
      if (tid == 0) write_no_box(p, inst, LA3D_BOX_UNSUPPORTED, 0.0, NAN);
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
    // (stays in the kernel body: moved into a function, the compiler contracts the sums of M the other way round - it rounds
    // another product of each a*b + c*d + e*f -, and the records change in their last bits)
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
  // ---- phase 0: mask -> bit image in LDS (the decoders borrow the LDS of the tile list, which is built afterwards) ----
  int nmask = 0;
  if constexpr (LDSMASK) nmask = mask_to_bits<VEC, SRC, FRAMES>(p, p_call, inst, mpl, bits, sh, list, TILED ? p.list_cap / 2 : 0, tid, wave, lane);
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
  if (SRC != 0 && LDSMASK && p.filter_boundary >= 0) {   // uniform: the fused keep rule - a dropped instance costs no passes
    if (!filter_keep<SRC>(p, sh, bits, inst_p, tid)) return;
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

  // ---- active-tile list; plain build (LK): the bit image compacted to the active tiles, and whether the instance takes the
  // separable single pass (sweep_sep): no ground rotation, no skew - x ray by column, y ray by row, z = depth ----
  constexpr bool LK = TILED && !SAMPLE;
  const bool sep_cam = LK && (HULL || !p.sep_off) && Mg[1] == 0.0 && Mg[3] == 0.0 && Mg[6] == 0.0 && Mg[7] == 0.0 && Mg[8] == 1.0;   // uniform
  TileList tiles;
  if (TILED && !sampled) {
    if constexpr (FRAMES) frame_rcp_ntx(p_frame);
    tiles = build_tile_list<LK>(p, sh, bits, list, sep_cam, tid, wave, lane);
    LA3D_STAMP(15);
    __syncthreads();
  }
  const int nactive = tiles.nactive, nfull = tiles.nfull, compact = tiles.compact;
  const bool sep = tiles.sep;

  if constexpr (HULL && LK) {   // hull call, full-mask mode: refused, rejected by the axis stage, or handed over to hull_finish_kernel
    hull_full_mask(sh, p, inst_p, dpl, bits, list, nactive, sep, Mg, nmask, wave, lane, cv);
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
      sample_pick<HULL, FRAMES, DepthT>(p, sh, bits, prefix, dpl, cv, Mg, ntot, my_draw, tid, wave, lane, acc, &cnt, &px, &py, &pz, &pok);
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
    if (tid_plain == 0) hull_handoff_header(hh, sh, 0.0, 0.0, 0.0, 0.0, (double)min(ntot, LA3D_NSAMPLE));
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
// The mask source of a call as a compile-time constant, handed to f: bit planes 3, run lengths 1, polygon parts 2 - the three that
// are decoded into the LDS bit image (DECODED: the caller's build has one) -, else the u8 plane, 0.  A frames call has no u8 plane
// (NO_U8): what is neither bit planes nor run lengths is polygon parts.
template <int SRC> using src_t = std::integral_constant<int, SRC>;
template <bool DECODED, bool NO_U8 = false, typename F>
int with_src(const KParams& p, F&& f) {
  if constexpr (DECODED) {
    if (p.mask_bits != nullptr) return f(src_t<3>());
    if (p.rle_counts != nullptr) return f(src_t<1>());
    if (NO_U8 || p.poly_xy != nullptr) return f(src_t<2>());
  }
  if constexpr (NO_U8) return LA3D_ERR_UNSUPPORTED;   // (not reached: a frames build is a DECODED one)
  else return f(src_t<0>());
}
// (a decoded source is always the 16-byte build: the bit image does not depend on the alignment of a u8 plane)
template <bool VEC, bool SAMPLE>
int launch_hull(const KParams& p, size_t lds, hipStream_t s) {
  return with_src<true>(p, [&](auto src) { return launch_hull_inst<VEC || decltype(src)::value != 0, SAMPLE, decltype(src)::value>(p, lds, s); });
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
  return with_src<LDSMASK>(p, [&](auto src) { return launch_fit_inst<VEC, LDSMASK, SAMPLE, TILED, decltype(src)::value>(p, lds, s, workspace); });
}

// la3d_fit_instances_frames / la3d_fit_instances_frames_depth16: run lengths or polygon parts, la3d_fit_instances_frames_bits: bit
// planes - the tiled form (full-mask or subsample)
template <bool SAMPLE>
int launch_fit_frames(const KParams& p, size_t lds, hipStream_t s, void* workspace) {
  return with_src<true, true>(p, [&](auto src) { return launch_fit_inst<true, true, SAMPLE, true, decltype(src)::value, true>(p, lds, s, workspace); });
}

}  // namespace

namespace la3d {
int LA3D_INSTANCE_FIT(KParams p, const CallFacts& f, hipStream_t s, void* workspace, const char* who) {
  const int H = p.H, W = p.W, B = p.B;
  const bool vec = f.vec, ldsmask = f.ldsmask;
  if (f.sample && !ldsmask) return refuse(who, "reference-subsample mode needs the bit image in LDS (H*W <= 1048576)", LA3D_ERR_UNSUPPORTED);
  // LDS per workgroup: bit image + Shared (f.lds), and behind them ONE area that the tile list, the rank prefix of the subsample mode
  // (one word per 32-word block of the bit image) and the polygon side stage share
  const size_t blocks = f.sample ? (size_t)rank_prefix_bytes(p.nwords) : 0;
  auto lds_with = [&](size_t list_bytes) { return f.lds + std::max({list_bytes, blocks, f.poly_stage}); };
  // tiled fast path: 32-px-wide tiles map to exactly one bit-image word / one 128-B depth line per row
  p.ntx = W / 32; p.nty = (H + 7) / 8;
  // ty = int((t + 0.5f) * rcp_ntx) is exact for t < 65536: the fraction of (t+0.5)/ntx stays at least 0.5/ntx away from
  // an integer and the float error is below (65536/ntx) * 1.2e-7
  p.rcp_ntx = 1.0f / (float)(p.ntx > 0 ? p.ntx : 1);
  p.tiles_per_wave = (p.ntx * p.nty + NWAVE - 1) / NWAVE;
  const bool tiled_frame = ldsmask && vec && W % 32 == 0 && p.ntx <= 255 && p.nty <= 255;
  if (f.sample) {
    if (lds_with(0) > 160 * 1024 - 256) return refuse(who, "reference-subsample mode: frame too large for LDS", LA3D_ERR_UNSUPPORTED);
    if (f.method == LA3D_METHOD_CONVEX_HULL) {   // every instance goes the sampled way: no tile list
      p.geo = static_cast<double*>(f.hull_area);
      return vec ? launch_hull<true, true>(p, lds_with(0), s) : launch_hull<false, true>(p, lds_with(0), s);
    }
    if (tiled_frame) {
      // masks of <= 500 px (not sampled) walk their active tiles; the list shares the LDS of the block prefix
      int budget = 0;                                          // four workgroups per CU if the frame allows (tiled_list_cap)
      const long cap = tiled_list_cap<true>(p.mask_lds_bytes, p.nwords, p.ntx * p.nty, &budget);
      if (cap >= 64 && budget <= 160 * 1024 - 256) {
        p.list_cap = (int)cap;
        if (f.frames) return launch_fit_frames<true>(p, lds_with((size_t)cap * 2), s, nullptr);
        return launch_fit<true, true, true, true>(p, lds_with((size_t)cap * 2), s);
      }
    }
    if (f.frames)
      return refuse(who, "reference-subsample mode: bounds outside the tiled form: H <= 2040, W <= 8160, and bit image + rank "
                         "prefix + 64 tile-list entries within one workgroup's LDS (160 KiB)", LA3D_ERR_UNSUPPORTED);
    return vec ? launch_fit<true, true, true>(p, lds_with(0), s) : launch_fit<false, true, true>(p, lds_with(0), s);
  }
  if (tiled_frame) {
    // the largest number of workgroups per CU (160 KiB LDS) that still leaves room for a useful list (tiled_list_cap); masks with
    // more active tiles than the cap take the dense walk
    const long cap = tiled_list_cap<false>(p.mask_lds_bytes, p.nwords, p.ntx * p.nty);
    if (cap >= 64) {
      p.list_cap = (int)cap;
      const size_t lds = lds_with((size_t)cap * 2);
      if (f.method == LA3D_METHOD_CONVEX_HULL) {
        p.geo = static_cast<double*>(f.hull_area);
        return launch_hull<true, false>(p, lds, s);
      }
      if (f.frames) return launch_fit_frames<false>(p, lds, s, workspace);
      if (p.mask != nullptr && B > 256) {
        // u8 planes: the resident groups start one group's stream time apart - 256 x H*W bytes at the ~6.4 TB/s a pure reader gets:
        // 12.3 us for 640x480 (the kernel applies it only under the size-ordered launch; LA3D_STAGGER_US overrides, 0 switches it
        // off).  Measured with the self-estimating launch (profiles/r04/r04_stagger.txt, run 4), us per call at 6 / 8 / 10 / 12 / 14 us:
        // config-2 masks B = 1024: 96.0 / 94.8 / 93.4 / 94.5 / 95.4, B = 1536: 130.4 / 127.4 / 124.9 / 125.0 / 124.3; config-5 masks
        // B = 1024: 84.8 / 82.5 / 80.4 / 78.1 / 77.5 - the config-2 optimum is 10, the skewed mix wants more: one stream time is between.
        double us = 256.0 * (double)p.HW / 6.4e6;
        if (config().stagger_us >= 0) us = config().stagger_us;
        p.stagger_ticks = (int)(us * 100.0);
      }
      return launch_fit<true, true, false, true>(p, lds, s, workspace);
    }
  }
  if (f.frames)
    return refuse(who, "bounds outside the tiled form: H <= 2040, W <= 8160, and bit image + 64 tile-list entries within one "
                       "workgroup's LDS (160 KiB)", LA3D_ERR_UNSUPPORTED);
  if (f.method == LA3D_METHOD_CONVEX_HULL) {
    // full-mask hull on a frame outside the tiled vector path: no per-column structure to take the hull from - every instance is
    // refused (LA3D_BOX_UNSUPPORTED); reference-subsample mode (sample_idx) covers such frames
    return hull_refuse_launch(p, s);
  }
  if (ldsmask) return vec ? launch_fit<true, true, false>(p, lds_with(0), s, workspace) : launch_fit<false, true, false>(p, lds_with(0), s);
  return vec ? launch_fit<true, false, false>(p, lds_with(0), s) : launch_fit<false, false, false>(p, lds_with(0), s);
}
}  // namespace la3d
