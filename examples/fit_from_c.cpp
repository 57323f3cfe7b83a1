// Driving the C-ABI of libla3d.so from a plain host program: no Python, no torch.
//   hipcc -O2 -I include examples/fit_from_c.cpp -L labelany3d_amd/lib -lla3d -Wl,-rpath,'$ORIGIN' -o labelany3d_amd/lib/fit_from_c
//   labelany3d_amd/lib/fit_from_c <B> <H> <W> <seed>
// Builds B synthetic instances (private depth planes, one rectangle each, a ground plane per instance) with a small
// LCG, runs la3d_fit_instances on HIP buffers and prints status + the 39 doubles of every record in hex-exact form
// ("%a"), then repeats the fit through la3d_fit_instances_ex (C struct argument block) with the 2-D boxes of the records ("P"
// lines), with the masks packed to bit planes, through la3d_fit_instances_bits and, with two frame sizes in one call, through
// la3d_fit_instances_frames.  tests/test_gpu_cabi.py regenerates the same inputs in NumPy and checks the printed records against the oracle.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "la3d.h"

static uint32_t lcg_state;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }   // 24 random bits
static double unit() { return (double)lcg() / 16777216.0; }

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: %s B H W seed\n", argv[0]); return 1; }
  const int B = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]);
  lcg_state = (uint32_t)atoi(argv[4]);
  const size_t HW = (size_t)H * W;
  std::vector<float> depth(B * HW);
  std::vector<uint8_t> mask(B * HW, 0);
  std::vector<double> ground(B * 4), K = {0.8 * W, 0, 0.5 * W, 0, 0.8 * W, 0.5 * H, 0, 0, 1};
  for (int i = 0; i < B; ++i) {
    for (size_t p = 0; p < HW; ++p) depth[i * HW + p] = (float)(0.5 + 9.5 * unit());
    const int h = 1 + (int)(lcg() % (uint32_t)H), w = 1 + (int)(lcg() % (uint32_t)W);
    const int r0 = (int)(lcg() % (uint32_t)(H - h + 1)), c0 = (int)(lcg() % (uint32_t)(W - w + 1));
    for (int r = r0; r < r0 + h; ++r)
      for (int c = c0; c < c0 + w; ++c) mask[i * HW + (size_t)r * W + c] = (uint8_t)(1 + i % 250);
    ground[i * 4 + 0] = 0.02 + 0.1 * (unit() - 0.5); ground[i * 4 + 1] = -0.98 + 0.1 * (unit() - 0.5);
    ground[i * 4 + 2] = 0.1 + 0.1 * (unit() - 0.5);  ground[i * 4 + 3] = 1.5;
  }
  if (la3d_version() != LA3D_ABI_VERSION) { fprintf(stderr, "ABI version mismatch\n"); return 3; }
  float* d_depth; uint8_t* d_mask; double *d_K, *d_ground, *d_out, *d_aux; int32_t* d_status; void* d_ws;
  const size_t ws = la3d_workspace_bytes(B, H, W);
  HIPCHK(hipMalloc(&d_depth, depth.size() * 4)); HIPCHK(hipMalloc(&d_mask, mask.size()));
  HIPCHK(hipMalloc(&d_K, 72)); HIPCHK(hipMalloc(&d_ground, ground.size() * 8));
  HIPCHK(hipMalloc(&d_out, (size_t)B * LA3D_REC * 8)); HIPCHK(hipMalloc(&d_aux, (size_t)B * LA3D_AUX * 8));
  HIPCHK(hipMalloc(&d_status, (size_t)B * 4)); HIPCHK(hipMalloc(&d_ws, ws ? ws : 8));
  HIPCHK(hipMemcpy(d_depth, depth.data(), depth.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_mask, mask.data(), mask.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_K, K.data(), 72, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_ground, ground.data(), ground.size() * 8, hipMemcpyHostToDevice));
  hipStream_t stream;
  HIPCHK(hipStreamCreate(&stream));
  const int rc = la3d_fit_instances(d_depth, (int64_t)HW, nullptr, d_mask, d_K, 0, d_ground, nullptr, B, H, W, d_out, d_status,
                                    d_aux, d_ws, stream);
  if (rc != LA3D_SUCCESS) { fprintf(stderr, "la3d_fit_instances: %d %s\n", rc, la3d_last_error()); return 4; }
  HIPCHK(hipStreamSynchronize(stream));
  std::vector<double> out((size_t)B * LA3D_REC);
  std::vector<int32_t> status(B);
  HIPCHK(hipMemcpy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(status.data(), d_status, (size_t)B * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < B; ++i) {
    printf("%d", status[i]);
    for (int k = 0; k < LA3D_REC; ++k) printf(" %a", out[(size_t)i * LA3D_REC + k]);
    printf("\n");
  }
  // the same fit through the extensible entry point, with the records' 2-D boxes from the same epilogue: the records must be
  // identical, and the boxes those of la3d_project_boxes on the finished records ("P" lines)
  {
    double *d_out2, *d_proj, *d_proj2;
    HIPCHK(hipMalloc(&d_out2, (size_t)B * LA3D_REC * 8)); HIPCHK(hipMalloc(&d_proj, (size_t)B * 64)); HIPCHK(hipMalloc(&d_proj2, (size_t)B * 64));
    la3d_fit_args a = {};
    a.struct_size = (int32_t)sizeof(a);
    a.B = B; a.H = H; a.W = W;
    a.depth = d_depth; a.depth_plane_stride = (int64_t)HW; a.mask = d_mask; a.K = d_K; a.k_stride = 0; a.ground = d_ground;
    // (a zero-initialised block means: no fused instance filter, no area hints, no 2-D boxes unless proj is set)
    a.proj = d_proj; a.image_width = W; a.image_height = H;
    a.out = d_out2; a.status = d_status; a.aux = d_aux; a.workspace = d_ws; a.stream = stream;
    if (la3d_fit_instances_ex(&a) != LA3D_SUCCESS) { fprintf(stderr, "la3d_fit_instances_ex: %s\n", la3d_last_error()); return 6; }
    if (la3d_project_boxes(d_out2, d_K, 0, nullptr, B, (double)W, (double)H, d_proj2, stream) != LA3D_SUCCESS) return 7;
    HIPCHK(hipStreamSynchronize(stream));
    std::vector<double> out2(out.size()), pr((size_t)B * 8), pr2((size_t)B * 8);
    HIPCHK(hipMemcpy(out2.data(), d_out2, out2.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pr.data(), d_proj, pr.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pr2.data(), d_proj2, pr2.size() * 8, hipMemcpyDeviceToHost));
    if (memcmp(out.data(), out2.data(), out.size() * 8) != 0) { fprintf(stderr, "la3d_fit_instances_ex: records differ\n"); return 8; }
    if (memcmp(pr.data(), pr2.data(), pr.size() * 8) != 0) { fprintf(stderr, "la3d_fit_instances_ex: 2-D boxes differ from la3d_project_boxes\n"); return 9; }
    for (int i = 0; i < B; ++i) {
      printf("P");
      for (int k = 0; k < 8; ++k) printf(" %a", pr[(size_t)i * 8 + k]);
      printf("\n");
    }
    // the same masks once more as bit planes (1 bit per pixel, la3d.h "masks as bit planes"): packed on the device, then fitted
    // through the same block without its u8 pointer - same status, same records to rounding (another engine may have fitted the u8 call)
    {
      const size_t nw = la3d_mask_bits_words(H, W);
      uint32_t* d_bits;
      int32_t* d_status3;
      HIPCHK(hipMalloc(&d_bits, (size_t)B * nw * 4)); HIPCHK(hipMalloc(&d_status3, (size_t)B * 4));
      if (la3d_pack_mask_bits(d_mask, (int64_t)HW, B, H, W, W, d_bits, (int64_t)nw, stream) != LA3D_SUCCESS) { fprintf(stderr, "la3d_pack_mask_bits: %s\n", la3d_last_error()); return 11; }
      la3d_fit_args b = a;
      b.mask = nullptr; b.proj = nullptr; b.status = d_status3;
      if (la3d_fit_instances_bits(&b, d_bits, (int64_t)nw, LA3D_BITS_HEIGHT_ROWS) != LA3D_SUCCESS) { fprintf(stderr, "la3d_fit_instances_bits: %s\n", la3d_last_error()); return 12; }
      HIPCHK(hipStreamSynchronize(stream));
      std::vector<double> out3(out.size());
      std::vector<int32_t> status3(B);
      HIPCHK(hipMemcpy(out3.data(), d_out2, out3.size() * 8, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(status3.data(), d_status3, (size_t)B * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < B; ++i) {
        bool same = status3[i] == status[i];
        for (int k = 0; same && status[i] == LA3D_BOX_OK && k < 15; ++k) {
          const double x = out[(size_t)i * LA3D_REC + k], y = out3[(size_t)i * LA3D_REC + k];
          same = fabs(x - y) <= 1e-9 * (fabs(x) > 1.0 ? fabs(x) : 1.0);
        }
        if (!same) { fprintf(stderr, "la3d_fit_instances_bits: instance %d differs from the u8 call\n", i); return 13; }
      }
    }
    // images of two DIFFERENT sizes in ONE call (la3d.h "images of different sizes in one call"): frame 0 is plane 0 at H x W, frame 1
    // the upper left quarter of the last plane, both in one depth buffer at their own pitch (the next multiple of 32); instance i
    // belongs to frame i % 2, its rectangle - cut to the frame - goes in as column-major run lengths over the frame's own size.
    // Checked against one uniform call per frame size (la3d_fit_instances_ex with frame_width): same status, records to rounding.
    {
      const int fh[2] = {H, H > 1 ? H / 2 : 1}, fw[2] = {W, W > 1 ? W / 2 : 1}, src[2] = {0, B - 1};
      int pitch[2]; int64_t off[2]; size_t total = 0;
      for (int f = 0; f < 2; ++f) { pitch[f] = (fw[f] + 31) / 32 * 32; off[f] = (int64_t)total; total += (size_t)fh[f] * pitch[f]; }
      std::vector<float> fdepth(total, 0.0f);
      for (int f = 0; f < 2; ++f)
        for (int r = 0; r < fh[f]; ++r)
          for (int c = 0; c < fw[f]; ++c) fdepth[(size_t)off[f] + (size_t)r * pitch[f] + c] = depth[src[f] * HW + (size_t)r * W + c];
      std::vector<la3d_frame> table(2);
      for (int f = 0; f < 2; ++f) { table[f].depth_offset = off[f]; table[f].H = fh[f]; table[f].W = pitch[f]; table[f].frame_width = fw[f]; table[f].reserved = 0; }
      std::vector<int32_t> counts, index(B);
      std::vector<int64_t> offsets(B + 1, 0);
      for (int i = 0; i < B; ++i) {   // column-major runs of instance i's mask inside its frame, zeros first
        const int f = i % 2;
        index[i] = f;
        int run = 0, val = 0;
        for (int c = 0; c < fw[f]; ++c)
          for (int r = 0; r < fh[f]; ++r) {
            const int v = mask[i * HW + (size_t)r * W + c] != 0;
            if (v != val) { counts.push_back(run); run = 0; val = v; }
            ++run;
          }
        counts.push_back(run);
        offsets[i + 1] = (int64_t)counts.size();
      }
      float* d_fdepth; la3d_frame* d_table; int32_t *d_counts, *d_index, *d_status4; int64_t* d_offsets; double* d_out4;
      HIPCHK(hipMalloc(&d_fdepth, total * 4)); HIPCHK(hipMalloc(&d_table, sizeof(la3d_frame) * 2)); HIPCHK(hipMalloc(&d_counts, counts.size() * 4));
      HIPCHK(hipMalloc(&d_index, (size_t)B * 4)); HIPCHK(hipMalloc(&d_offsets, (size_t)(B + 1) * 8)); HIPCHK(hipMalloc(&d_status4, (size_t)B * 4));
      HIPCHK(hipMalloc(&d_out4, (size_t)B * LA3D_REC * 8));
      HIPCHK(hipMemcpy(d_fdepth, fdepth.data(), total * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(d_table, table.data(), sizeof(la3d_frame) * 2, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(d_counts, counts.data(), counts.size() * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(d_index, index.data(), (size_t)B * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(d_offsets, offsets.data(), (size_t)(B + 1) * 8, hipMemcpyHostToDevice));
      la3d_fit_args m = {};
      m.struct_size = (int32_t)sizeof(m);
      m.B = B; m.H = fh[0]; m.W = pitch[0];                 // the bounds: the largest rows, the largest pitch
      m.depth = d_fdepth; m.image_index = d_index; m.rle_counts = d_counts; m.rle_offsets = d_offsets; m.K = d_K; m.ground = d_ground;
      m.out = d_out4; m.status = d_status4; m.stream = stream;
      void* d_ws4;
      const size_t ws4 = la3d_fit_workspace_bytes(&m);
      HIPCHK(hipMalloc(&d_ws4, ws4 ? ws4 : 8));
      m.workspace = d_ws4;
      if (la3d_fit_instances_frames(&m, d_table, 2) != LA3D_SUCCESS) { fprintf(stderr, "la3d_fit_instances_frames: %s\n", la3d_last_error()); return 14; }
      HIPCHK(hipStreamSynchronize(stream));
      std::vector<double> out4((size_t)B * LA3D_REC), out5((size_t)B * LA3D_REC);
      std::vector<int32_t> status4(B), status5(B);
      HIPCHK(hipMemcpy(out4.data(), d_out4, out4.size() * 8, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(status4.data(), d_status4, (size_t)B * 4, hipMemcpyDeviceToHost));
      for (int f = 0; f < 2; ++f) {   // the uniform entry, one call per frame size, on the instances of that frame
        std::vector<int32_t> cf;
        std::vector<int64_t> of(1, 0);
        std::vector<double> gf;
        std::vector<int> ids;
        for (int i = f; i < B; i += 2) {
          cf.insert(cf.end(), counts.begin() + offsets[i], counts.begin() + offsets[i + 1]);
          of.push_back((int64_t)cf.size());
          gf.insert(gf.end(), ground.begin() + i * 4, ground.begin() + i * 4 + 4);
          ids.push_back(i);
        }
        const int Bf = (int)ids.size();
        if (Bf == 0) continue;
        HIPCHK(hipMemcpy(d_counts, cf.data(), cf.size() * 4, hipMemcpyHostToDevice));      // (the buffers of the mixed call are large enough)
        HIPCHK(hipMemcpy(d_offsets, of.data(), of.size() * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_out2, gf.data(), gf.size() * 8, hipMemcpyHostToDevice));        // (d_out2 is free by now: the sub-batch's ground rows)
        la3d_fit_args u = m;
        u.B = Bf; u.H = fh[f]; u.W = pitch[f]; u.frame_width = fw[f] == pitch[f] ? 0 : fw[f];
        u.depth = d_fdepth + off[f]; u.image_index = nullptr; u.depth_plane_stride = 0; u.ground = d_out2;
        if (la3d_fit_instances_ex(&u) != LA3D_SUCCESS) { fprintf(stderr, "la3d_fit_instances_ex (frame %d): %s\n", f, la3d_last_error()); return 15; }
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipMemcpy(out5.data(), d_out4, (size_t)Bf * LA3D_REC * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(status5.data(), d_status4, (size_t)Bf * 4, hipMemcpyDeviceToHost));
        for (int n = 0; n < Bf; ++n) {
          const int i = ids[n];
          bool same = status5[n] == status4[i];
          for (int k = 0; same && status4[i] == LA3D_BOX_OK && k < 15; ++k) {
            const double x = out4[(size_t)i * LA3D_REC + k], y = out5[(size_t)n * LA3D_REC + k];
            same = fabs(x - y) <= 1e-9 * (fabs(x) > 1.0 ? fabs(x) : 1.0);
          }
          if (!same) { fprintf(stderr, "la3d_fit_instances_frames: instance %d differs from the uniform call of its frame size\n", i); return 16; }
        }
      }
    }
    a.struct_size = 8;   // a truncated argument block is an error, not a crash
    if (la3d_fit_instances_ex(&a) != LA3D_ERR_ARG) { fprintf(stderr, "expected LA3D_ERR_ARG for a short struct\n"); return 10; }
  }
  // a bad call must come back as an error code, not a crash
  if (la3d_fit_instances(nullptr, (int64_t)HW, nullptr, d_mask, d_K, 0, nullptr, nullptr, B, H, W, d_out, d_status, nullptr,
                         d_ws, stream) != LA3D_ERR_ARG) { fprintf(stderr, "expected LA3D_ERR_ARG\n"); return 5; }
  return 0;
}
