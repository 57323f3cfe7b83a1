// la3d_engines.hpp - what the fit engines (one translation unit each) offer la3d_fit_instances' dispatcher (la3d.hip), and the
// launch helpers they share.  Host side only.  Each engine says which calls its kernels can take (*_applies: no pins, no batch
// limits - which engine fits a call is decided in one place, choose_engine in la3d.hip) and launches them (*_fit).
#pragma once
#include <chrono>

#include "la3d_device.hpp"

namespace la3d {
// What fit_dispatch works out once per call, beside the kernel argument FitParams
struct CallFacts {
  bool vec;            // 16-byte vector path: every plane base 16-aligned, H*W % 16 == 0
  bool ldsmask;        // the bit image fits LDS (FitParams::mask_lds_bytes > 0)
  bool sample;         // reference-subsample mode (sample_idx given)
  size_t lds;          // bit image + Shared
  size_t poly_stage;   // polygon input: the side stage behind Shared, else 0
  int method = 0;      // LA3D_METHOD_*: a convex-hull call (la3d_fit_args::method) runs on the instance engine only
  bool frames = false; // la3d_fit_instances_frames: frames of different sizes (FitParams::frames), the instance engine's tiled form only
  void* hull_area = nullptr;   // hull call: the hand-off area behind the first la3d_workspace_bytes(B,H,W) bytes of the workspace
};

// instance engine (la3d_instance.hip): one workgroup per instance - takes every call; picks the instantiation of
// fit_instances_kernel for the frame and launches it
int instance_fit(FitParams p, const CallFacts& f, hipStream_t s, void* workspace, const char* who);
// the same engine on 16-bit depth planes (la3d_instance_f16.hip / la3d_instance_u16.hip: la3d_instance.hip compiled for IEEE half /
// uint16 x scale elements; la3d_fit_instances_depth16)
int instance_fit_f16(FitParams16 p, const CallFacts& f, hipStream_t s, void* workspace, const char* who);
int instance_fit_u16(FitParams16 p, const CallFacts& f, hipStream_t s, void* workspace, const char* who);
// the launches behind the fit kernel of a hull call, which read no depth (la3d_hull_finish.hip: one unit, shared by the three instance units)
int hull_finish_launch(const FitParams& p, bool sample, hipStream_t s);
int hull_refuse_launch(const FitParams& p, hipStream_t s);
// band engine (la3d_band.hip): two / four / eight workgroups per instance that meet through the workspace
bool band_applies(const FitParams& p, const CallFacts& f);
bool band_frame_ok(int H, int W, int nb);
size_t band_workspace_bytes(int B);
int band_fit(const FitParams& p, hipStream_t s, void* workspace);
// row engine (la3d_rows.hip): up to sixteen workgroups per instance, one per band of rows.  two_launch: fit_rows_kernel, then
// merge_rows_kernel, instead of the one launch in which the last band to arrive merges its instance
bool rows_applies(const FitParams& p, const CallFacts& f);
int rows_fit(const FitParams& p, bool two_launch, hipStream_t s, void* workspace);
size_t rows_workspace_bytes(int B, int H, int W);
// split engine (la3d_split.hip): scan -> plan -> walk -> axis -> walk -> final over tile ranges
bool split_applies(const FitParams& p, const CallFacts& f);
int split_fit(const FitParams& p, void* workspace, hipStream_t s);
size_t split_workspace_bytes(int B, int H, int W);

// Is s capturing into a HIP graph?  (A failed query counts as capturing: the caller then takes its replay-safe form.)  A call
// captured into a graph replays with the tags and nonces of its capture, so the engines that meet through tagged workspace words
// run differently when capturing.
inline bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
  (void)hipGetLastError();
  return capturing;
}

// 48-bit per-call tag of the tagged arrival words (tagged_arrive), never 0: zeroed words - a captured call's memset - never look
// like this call's
inline unsigned long long call_tag(const void* workspace) {
  const unsigned long long t = (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count();
  const unsigned long long tag = (((t * 0x9E3779B97F4A7C15ull) >> 13) ^ (unsigned long long)reinterpret_cast<uintptr_t>(workspace)) & 0xffffffffffffull;
  return tag == 0 ? 1 : tag;
}
}  // namespace la3d
