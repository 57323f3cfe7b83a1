// la3d_bitplanes.hpp - what the units that read or write bit planes share (la3d_bits.hip: decoders, packers, unpacker, statistics;
// la3d_rle_encode.hip: the run-length encoder; la3d_open.hip: the opening; la3d_components.hip: connected components;
// la3d_cloud.hip: the prologue; la3d_overlap.hip: at() and the offset rule).
// Device side: where the planes of a call lie (BitsOut), the geometry of one of them (plane_geometry), the prologue of a frames
// workgroup (frames_prologue) and, for a frames call that reads planes and may write planes, its planes and their locator
// (FramesPlanes, frames_source, frames_dest: the end-inside-the-buffer checks behind the prologue); the rule of a plane offset
// (plane_offset_ok) and the realigned word of an image row (plane_row_word).  Host side: how an entry describes its planes
// (bits_out_uniform / bits_out_frames), the ONE argument check of the packer entries (pack_check), the in-place rule (planes_overlap)
// and the wording more than one unit uses.  (Refusals: refuse, la3d_device.hpp.)
// A BitsOut describes the planes of ONE call, in the uniform form (stride) or the frames form (offsets, frames, image_index):
//   as a DESTINATION (every packer) the kernels store the words of instance b's plane through `bits` and, where the entry has one,
//     its popcount to area[b];
//   as a SOURCE (the run-length encoder) the same fields say where the planes are READ: the kernels only load through `bits`, `area`
//     is NULL, and the entry that fills it in casts its const pointer once.  pack_check applies the same rules to either.
#pragma once
#include <initializer_list>

#include "la3d_device.hpp"
#include "la3d_poly.hpp"

using namespace la3d;

namespace {
constexpr int NT_DEC = 512;   // decode kernels: 8 waves per workgroup (four workgroups per CU by LDS: 32 waves keep the stores coming)

struct BitsOut {              // where the planes of a call go (kernel argument)
  unsigned* bits;
  long long stride;           // uniform form: words between planes
  const long long* offsets;   // frames form: words from bits to the plane of each instance
  int* area;                  // [B] or NULL
  const la3d_frame* frames;   // frames form: the table, P rows
  const int* image_index;
  int P;
  int H, W;                   // uniform form: the frame as stored (W = W_out); frames form: the bounds
  int frame_w;                // uniform form: the image columns where the rows are padded (0: none)
  int lds_words;              // words of the bit image the launch reserved (uniform form: the plane's)
  int vec;                    // uniform form: every plane 16-byte aligned
};
struct PlaneGeo { int H, W, fw, nwords, vec; unsigned* out; };

// ---- the prologue of a frames packer's workgroup, stated once ------------------------------------------------------------------
// Every value that decides whether and where something is read or written is wave-uniform, comes through a scalar load and is checked
// BEFORE an address is formed from it.  The order of the steps is the safety property:
//   1  BY_INSTANCE: image_index[n] inside [0, P) - before the frame row is addressed (else n IS the image: the grid's own)
//   2  the frame row keeps the contract (frame_row_ok: the check the fit makes) - before anything is read or written through it
//   3  BY_INSTANCE: the plane's offset >= 0 and a multiple of 4 (frames_plane_at: the rule of the fit)
//   4  nwords = H * W / 32   (<= the bounds' plane: H <= max_h, W <= max_w, W % 32 == 0)
//   5  CHUNKED (one lane per word, 256 words per chunk): a chunk beyond the plane's words - before any load; then the lane's word w,
//      live = w < nwords, have = the bits of word w that are image columns (0 where not live)
// false: refused - nothing is read, nothing is written.
// (The text below is shaped by the instruction streams of its four users, which are those they had with a prologue each: the row is
// checked as a local and stored afterwards - checked in place, the annotation packers lose `0 < fw <= W` and clip again -, and the
// plane is given both as a pointer and as words from bits, because pack_*_bits_kernel forms bits + off here and the others off + w.)
struct FramesWork { FrameRow r; unsigned* out; long long off; int nwords, w; bool live; unsigned have; };   // out = bits + off: the plane

// the bits of word w of a plane W wide that are columns < fw (a row is a whole number of words)
__device__ inline unsigned image_columns(int w, int W, int fw) {
  const int rem = fw - (w % (W >> 5)) * 32;
  return rem >= 32 ? 0xffffffffu : rem <= 0 ? 0u : (1u << rem) - 1u;
}
// the rule of a plane's offset, in words from its buffer: >= 0 and a multiple of 4 (a 16-byte aligned plane) - the rule of the fit
__device__ inline bool plane_offset_ok(long long off) { return off >= 0 && (off & 3) == 0; }
__device__ inline bool frames_plane_at(const long long* __restrict__ offsets, int b, long long* off) {
  const long long oo = uniform_i64(offsets[b]);
  if (!plane_offset_ok(oo)) return false;
  *off = oo;
  return true;
}
template <bool BY_INSTANCE, bool CHUNKED>
__device__ inline bool frames_prologue(const la3d_frame* frames, int P, const int* image_index, int max_h, int max_w, unsigned* bits,
                                       const long long* offsets, int n, int chunk, FramesWork* f) {
  int img = n;
  if constexpr (BY_INSTANCE) {
    img = __builtin_amdgcn_readfirstlane(image_index[n]);
    if ((unsigned)img >= (unsigned)P) return false;
  }
  const FrameRow r = frame_row_load(frames + img);
  if (!frame_row_ok(r, max_h, max_w)) return false;
  if constexpr (BY_INSTANCE) {
    if (!frames_plane_at(offsets, n, &f->off)) return false;
    f->out = bits + f->off;
  }
  f->r = r;
  f->nwords = (r.H * r.W) >> 5;
  if constexpr (CHUNKED) {
    if (chunk * 256 >= f->nwords) return false;
    f->w = chunk * 256 + (int)threadIdx.x;
    f->live = f->w < f->nwords;
    f->have = f->live ? image_columns(f->w, r.W, r.fw) : 0u;
  }
  return true;
}

// ---- the plane locator of a frames call that reads planes and may write planes (opening, components) ---------------------------
// The planes of such a call (kernel argument): row b reads the plane `offsets[b]` words into a buffer of `bits_words` words and, where
// the call stores planes, writes the one `out_offsets[b]` words into a buffer of `out_words`.
struct FramesPlanes {
  const long long* offsets; const long long* out_offsets;   // [B] words from the input / output buffer to the plane of each row
  const la3d_frame* frames; const int* image_index; int P;
  long long bits_words, out_words;         // words of the two buffers: a plane that does not end inside its buffer is refused
};
// Row b's SOURCE plane: steps 1 - 4 of frames_prologue (max_h, max_w: the bounds of the table), then that the plane ends inside its
// buffer `bits`.  The plane is the f->nwords words at bits + f->off: the caller forms that address, and only behind `true`.
__device__ inline bool frames_source(const FramesPlanes& c, const unsigned* bits, int max_h, int max_w, int b, FramesWork* f) {
  if (!frames_prologue<true, false>(c.frames, c.P, c.image_index, max_h, max_w, const_cast<unsigned*>(bits), c.offsets, b, 0, f)) return false;
  return f->off <= c.bits_words - f->nwords;
}
// Row b's DESTINATION plane of `words` words (the caller says how many its plane needs: it knows what it writes): the offset by the
// rule of step 3, then that the plane ends inside its buffer.  Called behind frames_source, and only where the call stores planes.
__device__ inline bool frames_dest(const FramesPlanes& c, int b, int words, long long* off) {
  if (!frames_plane_at(c.out_offsets, b, off)) return false;
  return *off <= c.out_words - words;
}

// the `valid` (>= 1; 32 or more: a whole word) columns from c0 on of image row v of a plane of pitch W, realigned so that column c0
// is bit 0; the bits above them are zero whatever the plane holds - a caller that passes no more than fw - c0 never sees a padding
// column.  nwords: the words of the plane - nothing beyond is read (N: the caller's type for it, which a word is indexed with).
template <typename N>
__device__ inline unsigned plane_row_word(const unsigned* __restrict__ plane, N nwords, int W, int v, int c0, int valid) {
  const long long i = (long long)v * W + c0;
  const N w = (N)(i >> 5);
  const unsigned sh = (unsigned)(i & 31);
  unsigned x = plane[w] >> sh;
  if (sh && w + 1 < nwords) x |= plane[w + 1] << (32 - sh);
  if (valid < 32) x &= (1u << valid) - 1u;
  return x;
}

// The geometry and the plane of instance b.  false (frames form): the instance is refused - nothing is written for it.
template <bool FRAMES>
__device__ inline bool plane_geometry(const BitsOut& c, int b, PlaneGeo* g) {
  if constexpr (FRAMES) {
    FramesWork f;
    if (!frames_prologue<true, false>(c.frames, c.P, c.image_index, c.H, c.W, c.bits, c.offsets, b, 0, &f)) return false;
    g->H = f.r.H; g->W = f.r.W; g->fw = f.r.fw;
    g->nwords = f.nwords;           // (<= lds_words)
    g->vec = 1;                     // (bits is 16-byte aligned - checked on the host - and the offset a multiple of 4)
    g->out = f.out;
  } else {
    g->H = c.H; g->W = c.W; g->fw = c.frame_w; g->nwords = c.lds_words; g->vec = c.vec;
    g->out = c.bits + (long long)b * c.stride;
  }
  return true;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
constexpr size_t ANN_LDS_MAX = 160 * 1024 - 256;

// the elements of a stored plane / the words of the bounds' plane of a frames call (rows of whole words); 0 for sizes the check refuses
inline long long plane_items(int H, int W_out) { return H > 0 && W_out > 0 ? (long long)H * W_out : 0; }
inline long long bounds_words(int H, int W) { return H > 0 && W > 0 ? (long long)H * (((long long)W + 31) / 32) : 0; }

// How an entry describes its destination - to pack_check, and to the kernels that take a BitsOut.
BitsOut bits_out_uniform(int H, int W, int W_out, uint32_t* bits, long long stride, int32_t* area) {
  BitsOut c = {};
  c.bits = bits; c.stride = stride; c.area = area;
  c.H = H; c.W = W_out; c.frame_w = W_out > W ? W : 0;
  c.lds_words = (int)la3d_mask_bits_words(H, W_out);
  c.vec = ((reinterpret_cast<uintptr_t>(bits) & 15) == 0 && stride % 4 == 0) ? 1 : 0;
  return c;
}
BitsOut bits_out_frames(const la3d_frame* frames, int P, int H, int W, const int32_t* image_index, uint32_t* bits, const int64_t* bits_offsets,
                        int32_t* area) {
  BitsOut c = {};
  c.bits = bits; c.offsets = reinterpret_cast<const long long*>(bits_offsets); c.area = area;
  c.frames = frames; c.image_index = image_index; c.P = P;
  c.H = H; c.W = W; c.lds_words = (int)bounds_words(H, W); c.vec = 1;
  return c;
}

inline uintptr_t at(const void* q) { return reinterpret_cast<uintptr_t>(q); }   // for the alignment and overlap rules an entry writes out
// the in-place rule of an entry that cannot work in place: do `in_words` words at `in` and `out_words` words at `out` share a byte?
inline bool planes_overlap(const void* in, uintptr_t in_words, const void* out, uintptr_t out_words) {
  return at(in) < at(out) + out_words * 4 && at(out) < at(in) + in_words * 4;
}

// The argument check of every packer entry.  The rules and their rank are the same for all of them and stated here, once; an entry
// brings its sizes, its pointers and ITS wording of each rule (the text of a refusal is part of the C ABI: two entries that phrase one
// rule differently keep their phrasing).  A rule whose wording is NULL does not exist for that entry.
//   1  sizes         B, P < 0, H, W <= 0, W_out < W                                    (P = 1: an entry without images)
//   2  shape         the entry's own bound on the frame and the grid: `shape_bad`
//   3  null_ptr      a pointer of the list that is not optional is NULL                 \ only where there is work to do
//   4  misaligned    (address & mask) != 0, pointer by pointer in the order of the list /
//   5  lds           the bit image does not fit LDS: `lds_bad` - LA3D_ERR_UNSUPPORTED, every other rule LA3D_ERR_ARG
//   6  src_stride    uniform form: the source's plane stride < H*W                      \ only where there is work to do
//   7  bits_stride   uniform form: out.stride < la3d_mask_bits_words(H, W_out)          /   (the frames form has neither)
// Returns the refusal's code (la3d_last_error() is set), PACK_NOTHING (the call is valid and has no work: success) or PACK_LAUNCH.
enum { PACK_LAUNCH = 0, PACK_NOTHING = 1 };
struct PackWords { const char *sizes, *shape, *null_ptr, *lds, *src_stride, *bits_stride; };
struct PackPtr { const void* p; unsigned mask; const char* misaligned; bool optional = false; };

int pack_check(const char* who, const PackWords& say, int B, int P, int W, bool work, bool shape_bad, bool lds_bad,
               std::initializer_list<PackPtr> ptrs, long long src_stride, const BitsOut& out) {
  if (B < 0 || P < 0 || out.H <= 0 || W <= 0 || out.W < W) return refuse(who, say.sizes);
  if (say.shape && shape_bad) return refuse(who, say.shape);
  if (work) {
    for (const PackPtr& q : ptrs)
      if (!q.p && !q.optional) return refuse(who, say.null_ptr);
    for (const PackPtr& q : ptrs)
      if (reinterpret_cast<uintptr_t>(q.p) & q.mask) return refuse(who, q.misaligned);
  }
  if (say.lds && lds_bad) return refuse(who, say.lds, LA3D_ERR_UNSUPPORTED);
  if (work && say.src_stride && src_stride < (long long)out.H * W) return refuse(who, say.src_stride);
  if (work && say.bits_stride && out.stride < (long long)la3d_mask_bits_words(out.H, out.W)) return refuse(who, say.bits_stride);
  return work ? PACK_LAUNCH : PACK_NOTHING;
}
inline int pack_done(int rc) { return rc < 0 ? rc : LA3D_SUCCESS; }   // what an entry returns when pack_check said anything but PACK_LAUNCH

// wording more than one unit uses
const char* const SIZES_FRAMES = "bad argument (B, P >= 0, bounds H, W > 0)";
const char* const BITS_STRIDE = "bits_plane_stride is smaller than la3d_mask_bits_words(H, W_out)";
}  // namespace
