/* la3d.h — C-ABI of the MI355X-native LabelAny3D geometric hot path (libla3d.so, gfx950).
 *
 * The reference has no FFI layer: the path is three module-level Python/NumPy functions
 * resolved by name (reference src/batch_scripts/whole.py:10,15-16).  This ABI is what a
 * binding for that path calls; labelany3d_amd/{util,util_3dbox}.py bind it with ctypes and
 * keep the reference's Python signatures.
 *
 * Conventions
 *  - every `const T* dev` / `T* dev` argument is a DEVICE pointer (tensor.data_ptr());
 *    arguments documented as HOST are read synchronously before the call returns.
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *    asynchronous with respect to the host; the caller owns every buffer.
 *  - no call throws, allocates device memory or synchronises the device.
 *  - return value: LA3D_SUCCESS or a negative LA3D_ERR_*; la3d_last_error() gives text.
 *  - per-box failures (the reference's ValueError cases) are reported in `status[B]`,
 *    never as a failed call.
 */
#ifndef LA3D_H
#define LA3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LA3D_ABI_VERSION 2
#define LA3D_REC 39      /* doubles per box: center_cam[3] dimensions[3]=(dz,dy,dx) R_cam[9] bbox3D_cam[8][3] */
#define LA3D_AUX 4       /* doubles per box: yaw, n_valid, n_in (mask pixels / cloud points), eigen-gap (l1-l2)/l1;
                            with LA3D_METHOD_CONVEX_HULL aux[3] = -(hull vertices) when the hull decided the yaw
                            and stays >= 0 when the reference's PCA fallback was taken (:222-224).
                            The PCA axis is conditioned like 1 / gap.  gap == 0 says "axis unresolved - any yaw is as good":
                            an exact tie of the two eigenvalues or a footprint without any spread (every point at the same
                            (x', z'): the reference's own axis is then the SVD of rounding noise).  A footprint whose spread
                            is below ~1/360 of its distance from the origin of the sums - the raw second moments cancel to
                            rounding noise, kappa = (sum x^2 + sum z^2) / (n l1) > 2^17 - is resolved by a second moments
                            pass about the mean (every engine, every point-cloud kernel) and reports its true gap
                             */
#define LA3D_NSAMPLE 500 /* reference src/util_3dbox.py:123-125 */

/* call status */
#define LA3D_SUCCESS 0
#define LA3D_ERR_ARG (-1)
#define LA3D_ERR_UNSUPPORTED (-2)
#define LA3D_ERR_HIP (-3)

/* per-box status (int32) — the reference's error behaviour, src/util_3dbox.py */
#define LA3D_BOX_OK 0         /* a box was fitted                                                        */
#define LA3D_BOX_EMPTY 1      /* ValueError("No valid points after removing NaN values")  (:142-143)     */
#define LA3D_BOX_BAD_GROUND 2 /* ground parallel/antiparallel to [0,-1,0] or zero: NaN rotation (:37-55)   */
#define LA3D_BOX_TOO_FEW 3    /* one valid point: scikit-learn PCA(2) ValueError (:183-184)              */
#define LA3D_BOX_NONFINITE 4  /* +-inf coordinate reaches PCA: scikit-learn ValueError (:183-184)        */
#define LA3D_BOX_UNSUPPORTED 5 /* convex_hull on more than 2048 valid points (the reference feeds it <= 500); la3d_fit_args::method =
                                  LA3D_METHOD_CONVEX_HULL in full-mask mode on an instance it does not cover (see "convex-hull yaw") */
#define LA3D_BOX_FILTERED 6   /* dropped by the instance filter of the *_filtered entry points (src/util.py:375)        */

/* yaw method (reference src/util_3dbox.py:146-151) */
#define LA3D_METHOD_PCA 0
#define LA3D_METHOD_CONVEX_HULL 1
/* OR-ed into `method` of la3d_fit_points: the caller promises that no cloud has more than a few thousand rows to visit (after
 * sampling) - true for the reference's own calls (500 mesh samples per object).  PCA method: one WAVE per cloud instead of one
 * workgroup - no LDS, no barriers, four clouds per workgroup.  Larger clouds stay correct, only slow. */
#define LA3D_HINT_SMALL_CLOUDS 0x100
#define LA3D_HINT_HULL_512 0x200     /* OR into `method` (convex hull): no cloud holds more than 512 valid rows - the reference's own call path
                                        (<= 500 mesh samples) - so the kernel takes its small-LDS form (eight workgroups per CU instead of
                                        three); implied by a sample_idx array.  A cloud that breaks the promise gets LA3D_BOX_UNSUPPORTED. */

int la3d_version(void);
/* "LA3D_BUILD_INFO:<sha256 of the sources this library was compiled from>:<sha256 of the compile command>" - static storage. */
const char* la3d_build_info(void);
const char* la3d_last_error(void);

/* Replaces depth_to_points(depth, K, R, t) — reference src/util.py:52-75 (caller
 * src/batch_scripts/depth.py:154).  depth: dev f32 [H*W] (batch element 0, as the reference
 * returns only that, :75).  K9: HOST f64[9] row-major pixel intrinsics.  Rt12: HOST f64[12]
 * = R row-major (9) then t (3), or NULL for identity.  out: dev [H*W*3], f64 when
 * out_is_f64 != 0 (the reference's dtype) else f32.  u = column, v = row, no half-pixel. */
int la3d_unproject(const float* depth, const double* K9, const double* Rt12, int H, int W,
                   void* out, int out_is_f64, void* stream);

/* The same for P frames in one launch (a dataset stage unprojects every image: the reference loops over them,
 * src/batch_scripts/depth.py:138-160).  depth: dev f32 [P][H*W]; K: DEVICE f64, 9 per frame (k_stride >= 9) or one shared
 * matrix (k_stride 0), inverted in the kernel with the same elimination as the host routine of la3d_unproject;
 * Rt12 as above (shared by all frames) or NULL; out: dev [P][H*W*3]. */
int la3d_unproject_batch(const float* depth, const double* K, int32_t k_stride, const double* Rt12, int P, int H, int W,
                         void* out, int out_is_f64, void* stream);

/* Number of True pixels per mask plane: what the reference sees as in_pc.shape[0]
 * (src/util_3dbox.py:123) when fed pts[mask].  mask: dev u8 [B][H*W] (non-zero = True);
 * counts: dev i32 [B].  The host needs it to draw np.random.randint(0, N, 500). */
int la3d_mask_counts(const uint8_t* mask, int B, int H, int W, int32_t* counts, void* stream);

/* Depth rows padded on the right with zeros: src dev f32 [rows][W] -> dst dev f32 [rows][Wp] (Wp >= W, Wp % 4 == 0, dst 16-byte
 * aligned; rows = planes x H).  What la3d_fit_args::frame_width wants for frames whose width is not a multiple of 32 (run-length /
 * polygon masks on COCO's 427 / 500 / 375 / 333-wide images): Wp = the next multiple of 32. */
int la3d_pad_rows(const float* src, int64_t rows, int W, int Wp, float* dst, void* stream);

/* The library keeps NO mutable process state (re-entrant, no global state).  How a call is scheduled - which
 * engine, whether the size-balanced launch order runs, which build of the instance kernel - is decided per call from its
 * arguments; the three `opt_*` fields of la3d_fit_args override the decision for one call (0 = the library's choice).  The
 * LA3D_* environment variables the measurement scripts use (LA3D_ENGINE, LA3D_BALANCE, LA3D_BUILD, ...) are read ONCE, at
 * the first call, into an immutable table of process defaults; they never change records, only speed.
 * (ABI 2: la3d_set_launch_order / la3d_get_launch_order of ABI 1 - a process-wide switch - are gone; use opt_launch_order.) */
/* Which engine fits a call: the engines are tried in the order rows -> band -> split -> instance, each where it applies and - by
 * default - up to its batch limit (160 instances each; LA3D_ROWS_MAXB moves the row engine's).  A pinned engine starts the walk at
 * itself and has no batch limit; where it does not apply the walk goes on to the engines after it, under their own limits - a
 * pinned rows engine may give way to the band engine, a pinned band engine to the split engine -, and the instance engine takes
 * what is left.  A call
 * without a ground array on a frame the single pass covers that the row engine does not take goes to the instance engine unless
 * band or split is pinned. */
#define LA3D_ENGINE_DEFAULT 0
#define LA3D_ENGINE_INSTANCE 1        /* one workgroup per instance: takes every call */
#define LA3D_ENGINE_SPLIT 2           /* band scan + tile-range-balanced passes (16-byte aligned, word-aligned rows, no subsample mode, no
                                         padded rows; run-length / polygon masks without the fused filter) */
#define LA3D_ENGINE_BAND 3            /* two, four or eight workgroups per instance, one per band of tile rows (u8 planes, tiled frames, no
                                         subsample mode) */
#define LA3D_ENGINE_ROWS 4            /* up to sixteen workgroups per instance, one per band of rows (u8 planes, no ground array, the
                                         default build, no subsample mode).  Taken by default for batches of up to 160 instances
                                         (LA3D_ROWS_MAXB), and up to 512 when pinned.  Round 6: ONE launch - the band that finishes last
                                         merges its instance's partial sums and writes the record */
#define LA3D_ENGINE_ROWS2 5           /* the row engine in its round-5 form: the partial sums merged by a second short launch (what a call
                                         captured into a HIP graph takes anyway) */
#define LA3D_ORDER_DEFAULT 0          /* size-balanced launch order for 256 < B <= 3 resident sets; the sort keys are estimated inside the
                                         fit kernel and handed over through the workspace, so ONE workspace serves ONE call at a time, and
                                         several ORDERED calls running concurrently on different streams slow each other down (a call whose
                                         workgroups are not all resident waits ~0.25 ms before computing its neighbours' keys itself):
                                         pipelined callers pass LA3D_ORDER_OFF, as labelany3d_amd/pipeline.py does */
#define LA3D_ORDER_OFF 1              /* a caller pipelining independent batches on several streams wants it off (measured +20 %) */
#define LA3D_ORDER_ON 2
#define LA3D_BUILD_DEFAULT 0          /* 64 VGPRs, four workgroups per CU; un-grounded, skew-free cameras take the separable SINGLE pass
                                         (round 5: one walk over the depth, extents from per-column depth ranges), every other call two passes */
#define LA3D_BUILD_PLAIN 1            /* the same build pinned to its two-pass form (pass-B tile culling) for every camera */
#define LA3D_BUILD_NOCULL 2           /* the two-pass form that walks EVERY active tile in pass B (no culling plan): the reference the culling
                                         tests compare with, never faster */
#define LA3D_BUILD_RETAINING LA3D_BUILD_NOCULL   /* rounds 2-5: a 128-VGPR build that kept depth tiles in registers between the passes -
                                         fastest nowhere since round 4 (106 vs 81 us per 1024 instances) and deleted in round 6; the value
                                         stays accepted and now selects the no-cull build (the same records: it never culled) */

/* Bytes of device scratch la3d_fit_instances needs for (B,H,W); may be 0. */
size_t la3d_workspace_bytes(int B, int H, int W);

/* The composed hot path, batched:
 *     for n in range(B):
 *         img  = image_index[n] if image_index else n
 *         pts  = depth_to_points(depth[img][None], K[img])[mask[n]]     # src/util.py:52-75, :480-481
 *         out[n] = estimate_bbox(pts, None, ground[n], 'pca')          # src/util_3dbox.py:106-178
 *     ('convex_hull' instead of 'pca': la3d_fit_args::method of la3d_fit_instances_ex, see "convex-hull yaw" below)
 * depth        dev f32, planes of H*W floats, plane p at depth + p*depth_plane_stride
 *              (stride in floats; 0 = one shared plane)
 * image_index  dev i32 [B] or NULL (instance n uses plane n)
 * mask         dev u8 [B][H*W], non-zero = True (np.bool_ layout, src/util.py:367,382)
 * K            dev f64, 9 per image, image p at K + p*k_stride (k_stride 0 = shared, else >= 9)
 * ground       dev f64 [B][4] or NULL; only [:3] is used (src/util_3dbox.py:128-134); a row whose
 *              first component is NaN means "no ground" for that instance
 * sample_idx   dev i32 [B][500] or NULL.  NULL = full-mask mode (every masked pixel is used).
 *              Non-NULL = reference-subsample mode: for an instance with N > 500 masked pixels
 *              the 500 ranks (0 <= r < N, row-major order of True pixels) the reference would
 *              draw at :124 select the points; rows of instances with N <= 500 are ignored.
 * out          dev f64 [B][39]  (NaN where status != 0)
 * status       dev i32 [B]
 * aux          dev f64 [B][4] or NULL
 * workspace    dev scratch of la3d_workspace_bytes(B,H,W) bytes (may be NULL when that is 0) */
int la3d_fit_instances(const float* depth, int64_t depth_plane_stride, const int32_t* image_index,
                       const uint8_t* mask, const double* K, int32_t k_stride,
                       const double* ground, const int32_t* sample_idx,
                       int B, int H, int W, double* out, int32_t* status, double* aux,
                       void* workspace, void* stream);

/* ---- mask ingestion: the data format immediately upstream of the path -------------------
 * The reference decodes COCO / COCONut annotations to (H,W) bool arrays on the CPU with pycocotools
 * (mask_utils.decode, src/util.py:367,401-402; encoder src/download_coconut.py:167-175) and filters instances by
 * area / height / border truncation (src/util.py:291-335, :375).  Run lengths are over the (H,W) mask in
 * COLUMN-major order, alternating zeros / ones, zeros first. */

/* la3d_fit_instances with the masks given as run lengths: rle_counts dev i32 [total], rle_offsets dev i64 [B+1].
 * The runs are decoded straight into the kernel's LDS bit image: no 1 B/px plane is ever materialised or read
 * (H*W <= 1048576).  All other arguments as la3d_fit_instances. */
int la3d_fit_instances_rle(const float* depth, int64_t depth_plane_stride, const int32_t* image_index,
                           const int32_t* rle_counts, const int64_t* rle_offsets, const double* K, int32_t k_stride,
                           const double* ground, const int32_t* sample_idx, int B, int H, int W,
                           double* out, int32_t* status, double* aux, void* workspace, void* stream);

/* mask_utils.decode for a batch: run lengths -> u8 planes mask_out dev [B][H*W] (0/1), H*W <= 1048576. */
int la3d_rle_decode(const int32_t* counts, const int64_t* offsets, int B, int H, int W, uint8_t* mask_out, void* stream);

/* Per mask plane (dev u8 [B][H*W]) the quantities of the reference's instance filter: stats dev i32 [B][4] =
 * area, rows holding a pixel (the RLE branch's height, :368-369), last-first+1 rows (get_maximum_height, :328-335),
 * pixels inside the four `boundary`-px border strips with corners counted twice (analyze_mask, :303-322). */
int la3d_mask_stats(const uint8_t* mask, int B, int H, int W, int boundary, int32_t* stats, void* stream);

/* The same four quantities straight from COCO run lengths (layout as la3d_fit_instances_rle), by interval arithmetic on
 * the runs: no mask plane is decoded.  Replaces mask_utils.decode + np.any/np.sum + analyze_mask for RLE annotations
 * (src/util.py:364-376).  H <= 32768, H*W <= 2^30. */
int la3d_mask_stats_rle(const int32_t* counts, const int64_t* offsets, int B, int H, int W, int boundary, int32_t* stats,
                        void* stream);

/* ---- polygon segmentations: the branch every kept COCONut instance takes in the reference -----------------------
 * create_boolean_mask_from_polygon (src/util.py:386-400; producer src/download_coconut.py:178-199, :275-280): every part
 * of a segmentation is truncated to int32 vertices (np.array(polygon).reshape(-1,2).astype(np.int32) — done by the
 * caller) and filled on its own with cv2.fillPoly(mask, [points], 1): OpenCV's drawing.cpp rule for 8-bit images,
 * LINE_8, shift 0 (sides drawn with the 8-connected LineIterator + even-odd scanline fill in 16.16 fixed point; parts
 * are OR-ed).  Layout: poly_xy dev i32 [total_points][2] (x, y); ring_offsets dev i64 [R+1] point offsets of the parts;
 * inst_rings dev i64 [B+1] part offsets of the instances (instance n = parts inst_rings[n]..inst_rings[n+1]).
 * Vertices may lie outside the frame (clipped like cv::clipLine).  H*W <= 1048576. */

/* la3d_fit_instances with the masks given as polygon parts, rasterised straight into the kernel's LDS bit image (no
 * 1 B/px plane exists anywhere).  All other arguments as la3d_fit_instances. */
int la3d_fit_instances_poly(const float* depth, int64_t depth_plane_stride, const int32_t* image_index,
                            const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings,
                            const double* K, int32_t k_stride, const double* ground, const int32_t* sample_idx,
                            int B, int H, int W, double* out, int32_t* status, double* aux, void* workspace, void* stream);

/* ---- instance filter fused into the fit (reference read_bounding_boxes_segmentations, src/util.py:336-383) ----------
 * The reference keeps an annotation when  height / H > 0.0625  and fewer than `max_edge` (10) mask pixels lie in the
 * `boundary`-px (10) border strips  and  area >= `min_area` (100)  (:375; analyze_mask :291-326), with height = rows
 * holding a pixel for RLE annotations (:368-369) and last row - first row + 1 for polygons (get_maximum_height,
 * :328-335).  These entry points evaluate that rule on the bit image the fit kernel has just built - no second decode /
 * rasterisation pass - write the four statistics (area, rows, span, edge; as la3d_mask_stats*) to stats (dev i32 [B][4],
 * may be NULL) and fit only the kept instances; a dropped instance gets status LA3D_BOX_FILTERED and a NaN record. */
int la3d_fit_instances_rle_filtered(const float* depth, int64_t depth_plane_stride, const int32_t* image_index,
                                    const int32_t* rle_counts, const int64_t* rle_offsets, const double* K, int32_t k_stride,
                                    const double* ground, const int32_t* sample_idx, int B, int H, int W, int boundary,
                                    int min_area, int max_edge, double* out, int32_t* status, double* aux, int32_t* stats,
                                    void* workspace, void* stream);
int la3d_fit_instances_poly_filtered(const float* depth, int64_t depth_plane_stride, const int32_t* image_index,
                                     const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings,
                                     const double* K, int32_t k_stride, const double* ground, const int32_t* sample_idx, int B,
                                     int H, int W, int boundary, int min_area, int max_edge, double* out, int32_t* status,
                                     double* aux, int32_t* stats, void* workspace, void* stream);

/* ---- one extensible entry: every option of the fit calls above, plus the 2-D boxes of the records -----------------
 * Exactly one of mask / rle_counts(+rle_offsets) / poly_xy(+ring_offsets, inst_rings) gives the masks.  filter_boundary >= 0
 * together with filter_max_edge > 0 switches the fused instance filter on (run-length / polygon masks; see the *_filtered
 * entry points); a zero-initialised block (`la3d_fit_args a = {0}`) therefore means NO filter, and so does
 * filter_boundary = -1.  proj != NULL adds
 * la3d_project_boxes' output for every record - bbox2D_proj (4) and bbox2D_trunc (4), reference
 * src/tools/combine_results.py:105-108, :238-252 - written by the same epilogue that writes the record (rejected / dropped
 * instances: 8 NaNs); image_width / image_height are the clamp limits.  struct_size = sizeof(la3d_fit_args) of the caller:
 * fields beyond it are taken as zero, so the struct can grow. */
typedef struct la3d_fit_args {
  int32_t struct_size;
  int32_t B, H, W;
  const float* depth; int64_t depth_plane_stride; const int32_t* image_index;
  const uint8_t* mask;
  const int32_t* rle_counts; const int64_t* rle_offsets;
  const int32_t* poly_xy; const int64_t* ring_offsets; const int64_t* inst_rings;
  const double* K; int32_t k_stride;
  int32_t filter_boundary, filter_min_area, filter_max_edge;   /* filter_boundary < 0 or filter_max_edge <= 0: no filter */
  const double* ground; const int32_t* sample_idx;
  int32_t* stats;                                              /* [B][4] | NULL (filter) */
  double* proj; double image_width, image_height;              /* [B][8] | NULL */
  double* out; int32_t* status; double* aux;
  void* workspace; void* stream;
  /* --- fields added after the first publication (struct_size tells which the caller has) --- */
  const int32_t* area_hint;   /* dev i32 [B] | NULL: mask areas in pixels the caller already knows (annotation "area", the statistics of
                                 a preceding filter): the size-balanced launch order then needs no estimate pass over the masks.  A
                                 hint only orders the work - wrong values cost speed, never correctness. */
  /* --- ABI 2: per-call scheduling overrides (speed only, never records; 0 = the library's choice) --- */
  int32_t opt_engine;         /* LA3D_ENGINE_* */
  int32_t opt_launch_order;   /* LA3D_ORDER_* */
  int32_t opt_build;          /* LA3D_BUILD_* */
  int32_t frame_width;        /* round 5 (this field was `opt_reserved, must be 0`): 0 = W.  0 < frame_width < W: the planes are W pixels wide
                                 IN MEMORY, but only the first frame_width columns are image - rows padded on the right, e.g. to a
                                 multiple of 32, which is what the tiled / single-pass forms need (a 640 x 427 frame runs 4-5 x
                                 faster as H = 640, W = 448, frame_width = 427).  Run-length / polygon masks only: polygon sides are
                                 clipped to frame_width (cv2.fillPoly on the unpadded frame), run lengths are column-major and need
                                 nothing, the fused filter takes its right border from frame_width; K and the pixel coordinates are
                                 those of the unpadded frame.  With u8 planes the caller pads the planes with zeros and leaves 0. */
  int32_t method;             /* LA3D_METHOD_PCA (0: what a block without this field means) or LA3D_METHOD_CONVEX_HULL; anything else:
                                 LA3D_ERR_ARG.  See "convex-hull yaw" below. */
} la3d_fit_args;
int la3d_fit_instances_ex(const la3d_fit_args* args);

/* Convex-hull yaw for the depth + mask fit (la3d_fit_args::method = LA3D_METHOD_CONVEX_HULL; la3d_fit_instances_ex and
 * la3d_fit_annotations_host - the positional entries stay PCA):
 *     out[n] = estimate_bbox(pts, None, ground[n], 'convex_hull')        # src/util_3dbox.py:189-224
 * the minimum-area enclosing rectangle over the hull edges of the x/z footprint, the remedy for the L-shaped footprints a depth
 * map gives (only the camera-facing surfaces are seen, and their principal axis is the diagonal of the L).
 *  - reference-subsample mode (sample_idx given): every camera, every ground vector; the at most 500 points of an instance
 *    go through the hull.  Exactly the reference's call.
 *  - full-mask mode (sample_idx NULL): for an instance WITHOUT ground rotation (ground NULL or a NaN row) and a K without skew,
 *    on a frame the tiled single pass covers (W % 32 == 0, 16-byte aligned planes, H*W % 16 == 0, the column arrays fit behind
 *    the instance's tile list).  All points of pixel column u lie on one ray through the origin of the x/z plane, so only the
 *    nearest and the farthest valid depth of a column can be hull vertices: the hull of the whole mask is the hull of at most
 *    2 x (occupied columns) points.  NaN and infinite depths under the mask are dropped (as the reference and the PCA call
 *    drop them), negative depths are fitted.  Every other instance gets LA3D_BOX_UNSUPPORTED and a NaN record (NaN proj), never a
 *    PCA box.  The rule, in the order it is applied:
 *      1. the frame (the whole call): outside the tiled path - W % 32 != 0, H*W % 16 != 0, planes not 16-byte aligned, fewer than
 *         64 tiles of 32 x 8 pixels (W/32 * ceil(H/8)) - every instance is refused;
 *      2. the instance: a finite ground row (degenerate or not), a skewed K (K[0][1] != 0), or more ACTIVE TILES (tiles of 32 x 8
 *         pixels holding a mask pixel) than the frame has room for.  Room = the largest n with n x 32 B + 8 W bytes within the
 *         bit image's H W / 8 bytes (the column arrays behind the compacted tiles), n x 40 B + 384 B within them (the tiles with
 *         their range words), and n within the tile list the launch reserves.  The list has 2-byte entries and lies behind the bit
 *         image and 752 B of fixed state in a workgroup's share of the 160 KiB of LDS of a CU: (160 KiB / g rounded down to 16 B
 *         - bit image - 752 B) / 2 entries for the first g of 4, 3, 2, 1 workgroups per CU that gives min(256, tiles of the
 *         frame) of them, never more than the frame has tiles.  So: 28 of the 84 tiles of a 224 x 96 frame, 220 of the 300 of
 *         320 x 240, 904 of the 1200 of 640 x 480 (the list of four workgroups per CU; the column arrays alone would allow
 *         1040), none on 256 x 64.  These come BEFORE the reference's own rejections: an empty mask, a mask without a valid depth or
 *         a degenerate ground row gets status 5 here, not 1 / 2, when it is refused for one of them;
 *      3. the candidates: a column whose nearest and farthest valid depth are the same float gives ONE candidate, every other
 *         occupied column two (-0 and +0 are two floats); more than 2048 candidates are refused.  Frames up to 1024 columns
 *         never get there; on a wider frame a one-row mask over 1056 columns is fitted (1056 candidates), a two-row mask over
 *         1025 columns of differing depths is refused (2050).
 *    aux of a refused instance: yaw and aux[3] NaN; n_valid 0 and n_in NaN where rule 1 / 2 refused (before the mask was counted),
 *    both exact where rule 3 did.  Use reference-subsample mode for what full-mask mode refuses.
 *  - the hull call runs on the instance engine, two launches on the caller's stream (fit -> hand-off through the workspace ->
 *    hull finish), capturable into a HIP graph.  opt_engine pins give way; opt_build values / process defaults that switch the
 *    single pass off (LA3D_BUILD_PLAIN, LA3D_BUILD_NOCULL) are speed options and are IGNORED by hull calls: they never turn a
 *    fitted box into a refusal.
 *  - aux = [yaw, n_valid, n_in, -(hull vertices)]; aux[3] >= 0 (the PCA gap) where the hull had fewer than 3 vertices and the
 *    reference's PCA fallback decided the yaw (:222-224).
 *  - workspace: la3d_fit_workspace_bytes(args) bytes - larger than la3d_workspace_bytes(B,H,W) for a hull call (the hand-off
 *    area), equal to it for a PCA call, 0 for B <= 0.  Only struct_size, B, H, W and method of the block are read. */
size_t la3d_fit_workspace_bytes(const la3d_fit_args* args);

/* ---- masks as bit planes ---------------------------------------------------------------------------------------------
 * The fit kernel turns every mask into a row-major, LSB-first bit image in LDS; a bit plane IS that image, 1 bit per pixel
 * (38 400 B instead of 307 200 B for 640x480), copied in without any decode.
 *
 * FORMAT.  Per instance one plane of nwords = la3d_mask_bits_words(H, W) = ceil(H*W / 32) uint32 words: pixel (v, u) of a frame
 * stored W pixels wide is bit (v*W + u) & 31 of word (v*W + u) >> 5 - np.packbits(mask.reshape(B, -1), axis=1,
 * bitorder="little") viewed as little-endian uint32.  Planes lie bits_plane_stride words apart (>= nwords; what lies between
 * two planes is never read as mask and never written by the packers).  Bits of the last word past H*W are ignored by every
 * kernel (cleared in LDS, not trusted).  Rows padded on the right (la3d_fit_args::frame_width, W % 32 == 0): the bits of
 * columns >= frame_width MUST be zero - the packers below guarantee it; a caller who packs by hand owns that.
 * The base must be 4-byte aligned; a 16-byte aligned base with bits_plane_stride % 4 == 0 streams in 16-byte groups.
 *
 * la3d_fit_instances_bits: la3d_fit_instances_ex with the masks given as bit planes.  args->mask, rle_counts and poly_xy must all
 * be NULL; every other field of the block means what it means there: ground, sample_idx, image_index, k_stride, filter_*, stats,
 * proj, area_hint, opt_*, frame_width, method (LA3D_METHOD_CONVEX_HULL included, with its workspace size), stream.  The call
 * runs on the instance engine at every batch size (opt_engine pins give way, as for hull calls).  Without area_hint the
 * size-balanced launch order takes its keys from an exact popcount of the planes.  H*W <= 1048576, else LA3D_ERR_UNSUPPORTED.
 * flags: the height rule of the fused filter (filter_boundary >= 0 and filter_max_edge > 0).  The reference has one per annotation
 * kind and a bit plane does not say where it came from: LA3D_BITS_HEIGHT_ROWS (0) = rows holding a pixel (run lengths,
 * src/util.py:368-369), LA3D_BITS_HEIGHT_SPAN = last row - first row + 1 (polygons, :328-335).  Other bits: LA3D_ERR_ARG. */
#define LA3D_BITS_HEIGHT_ROWS 0
#define LA3D_BITS_HEIGHT_SPAN 1
size_t la3d_mask_bits_words(int H, int W);   /* host, no device; 0 for H <= 0 or W <= 0 */
int la3d_fit_instances_bits(const la3d_fit_args* args, const uint32_t* mask_bits, int64_t bits_plane_stride, int32_t flags);

/* Packers (streaming kernels; any plane stride, any base alignment of the input: a general form stands behind the 16-byte form).
 * Output: B planes of la3d_mask_bits_words(H, W_out) words, bits_plane_stride words apart, rows padded from W to W_out >= W
 * columns with zero bits (W_out = W: none; the next multiple of 32 is what the tiled forms of the fit want).  Only the
 * words of a plane are written.
 * la3d_pack_mask_bits:   mask dev u8, plane b at mask + b*mask_plane_stride (bytes, >= H*W); non-zero byte -> 1.
 * la3d_pack_logits_bits: logits dev f32 / f16 / bf16 (LA3D_DTYPE_*), plane b at logits + b*plane_stride ELEMENTS; bit = x > threshold
 *                        (compared in float32; NaN -> 0, +inf -> 1 unless threshold is +inf, -inf -> 0).
 * la3d_unpack_mask_bits: planes stored W_in pixels wide -> mask dev u8 [B][H][W] (0 / 1), the first W <= W_in columns.
 * la3d_mask_stats_bits:  the four quantities of la3d_mask_stats per plane stored W pixels wide; frame_width (0 = W) = the image
 *                        columns, from which the right border strip is taken.  H*W <= 1048576. */
#define LA3D_DTYPE_F32 0
#define LA3D_DTYPE_F16 1
#define LA3D_DTYPE_BF16 2
int la3d_pack_mask_bits(const uint8_t* mask, int64_t mask_plane_stride, int B, int H, int W, int W_out, uint32_t* bits,
                        int64_t bits_plane_stride, void* stream);
int la3d_pack_logits_bits(const void* logits, int dtype, int64_t plane_stride, float threshold, int B, int H, int W, int W_out,
                          uint32_t* bits, int64_t bits_plane_stride, void* stream);
int la3d_unpack_mask_bits(const uint32_t* bits, int64_t bits_plane_stride, int B, int H, int W_in, int W, uint8_t* mask,
                          void* stream);
int la3d_mask_stats_bits(const uint32_t* bits, int64_t bits_plane_stride, int B, int H, int W, int frame_width, int boundary,
                         int32_t* stats, void* stream);

/* ---- masks as label maps ----------------------------------------------------------------------------------------------
 * The form instance masks have before they become planes, run lengths or polygons: ONE plane of segment ids per image (a panoptic
 * PNG, the output of a panoptic / entity segmentation network), every instance mask being `labels == id`.  la3d_pack_label_bits
 * turns P label planes into the B bit planes of the (image, id) rows the caller lists - the labels of an image are read once,
 * however many instances it has - and la3d_fit_instances_bits fits them (image_index = the image of each row).
 *
 * labels: dev, plane p at labels + p*plane_stride ELEMENTS (pixels for RGB8; >= H*W), rows W elements apart, aligned to the element.
 *   LA3D_LABEL_U8 / LA3D_LABEL_U16: zero-extended; LA3D_LABEL_I32: as it is; LA3D_LABEL_RGB8: 3 bytes per pixel,
 *   id = R + 256 G + 65536 B (the COCO panoptic PNG).
 * inst_offsets dev [P+1]: the instances of image p are the rows inst_offsets[p] .. inst_offsets[p+1]-1 (non-decreasing, from 0 to B;
 *   rows outside [0, B) are never touched); inst_label dev [B]: the id of each row.  An image without rows is never read.
 * VALUE.  Bit (v, u) of plane b = (label(image of b, v, u) == inst_label[b]), both sides as int32: an id outside the dtype's range
 *   matches nothing (an all-zero plane, not an error); rows that repeat an (image, id) pair each get the plane.
 * Output: B planes in exactly the format of la3d_pack_mask_bits (la3d_mask_bits_words(H, W_out) words each, bits_plane_stride words
 *   apart, rows padded from W to W_out >= W with zero bits; only the words of a plane are written, and every word of every plane).
 * area: dev [B] or NULL - the popcount of each plane (what area_hint and draw_sample_idx want); cleared by the call itself on
 *   `stream` (the call is capturable) and accumulated with one integer atomic per wave and instance.
 * LA3D_ERR_ARG: an unknown dtype, W_out < W, negative sizes, plane_stride < H*W, bits_plane_stride < la3d_mask_bits_words(H, W_out),
 *   misaligned pointers, NULL pointers with work to do.  B == 0 or P == 0: success, nothing is done.
 * A 16-byte form stands in front of a general one as for the packers above: U8 / U16 / I32 with W_out == W, H*W % 32 == 0 and every
 * label plane 16-byte aligned (base and stride) take it; everything else (RGB8 included) the general form. */
#define LA3D_LABEL_U8   0   /* zero-extended */
#define LA3D_LABEL_U16  1   /* zero-extended */
#define LA3D_LABEL_I32  2
#define LA3D_LABEL_RGB8 3   /* 3 bytes per pixel, id = R + 256 G + 65536 B (COCO panoptic PNG) */
int la3d_pack_label_bits(const void* labels, int dtype, int64_t plane_stride /* elements; pixels for RGB8 */,
                         int P, int H, int W, int W_out,
                         const int32_t* inst_offsets /* dev [P+1]: instances of image p are rows inst_offsets[p] .. inst_offsets[p+1]-1 */,
                         const int32_t* inst_label   /* dev [B] */, int B,
                         uint32_t* bits, int64_t bits_plane_stride, int32_t* area /* dev [B] or NULL */, void* stream);

/* ---- 16-bit depth planes ----------------------------------------------------------------------------------------------
 * Sensor depth is uint16 with a metric scale (millimetres: SUN RGB-D, ScanNet, ARKitScenes, every RealSense / Kinect stream); depth
 * networks run in half precision.  la3d_fit_instances_depth16 fits straight from such planes - no float32 copy is made or read.
 *
 * VALUES.  The float32 value the kernels fit for a stored 16-bit word x:
 *   LA3D_DTYPE_F16   float32(x): exact.  Subnormal halves, +-inf, NaN and -0 convert as IEEE says.
 *   LA3D_DTYPE_U16   float32(x) * scale: ONE float32 multiplication, rounded to float32 before any other use (never contracted
 *                    into a following fma).  With LA3D_DEPTH_ZERO_IS_HOLE a stored 0 becomes a quiet NaN: a hole, dropped exactly
 *                    as the float32 entries drop a NaN depth under the mask; without the flag 0 is the valid depth 0.0.
 * From that value on nothing changes: statuses, aux, proj, stats, the NaN / inf / negative-depth rules and the refusal rules of a
 * hull call apply to the up-converted value - a 16-bit call gives the records the float32 call gives on the up-converted planes
 * (to the rounding of a changed summation order where the engines differ, bit for bit against the instance engine).
 *
 * la3d_fit_instances_depth16(args, depth, mask_bits, bits_plane_stride, bits_flags):
 *   - args->depth must be NULL and args->depth_plane_stride 0: the planes come in `depth` (struct_size = sizeof(la3d_depth16)).
 *     planes: device pointer, 2-byte aligned; plane of instance n = image_index[n] or n, plane_stride ELEMENTS apart (>= H*W;
 *     0 = one shared plane).  Any 2-byte aligned base and any stride are fitted; an 8-byte aligned base with plane_stride % 4 == 0
 *     takes the vector forms (what a 16-byte aligned base and stride % 4 == 0 are to float32 planes).
 *   - the masks: exactly one of args->mask, args->rle_counts, args->poly_xy, or mask_bits != NULL with all three NULL;
 *     bits_plane_stride and bits_flags mean what they mean in la3d_fit_instances_bits (ignored when mask_bits is NULL).
 *   - every other field of the block means what it means in la3d_fit_instances_ex: ground, sample_idx, image_index, k_stride,
 *     filter_* + stats, proj, aux, area_hint, opt_*, frame_width, method (LA3D_METHOD_CONVEX_HULL included), stream.  Workspace:
 *     la3d_fit_workspace_bytes(args).
 *   - the call runs on the instance engine at every batch size (opt_engine pins give way, as for bit planes); the rows, band and
 *     split engines have no 16-bit form.  Every frame the float32 entry fits is fitted: the tiled form, the untiled forms, padded
 *     rows (frame_width).
 *   - refused before any launch (LA3D_ERR_ARG): NULL block or NULL planes, a bad struct_size, a dtype other than F16 / U16,
 *     args->depth != NULL or depth_plane_stride != 0, a U16 scale that is not finite or <= 0, flags set for F16 or unknown flag
 *     bits, no mask source or two of them.
 * la3d_fit_instances_frames takes float32 planes; its 16-bit form is la3d_fit_instances_frames_depth16 (below, "images of different
 * sizes in one call").  la3d_fit_annotations_host and the positional entries take float32 planes only.
 *
 * Packers (streaming kernels; any plane stride, any element alignment):
 *   la3d_pack_depth16    depth dev f32, plane p at depth + p*plane_stride floats -> planes of H x W_out 16-bit words, out_plane_stride
 *                        ELEMENTS apart, rows padded from W to W_out >= W columns with zeros; only the words of a plane are written.
 *                        F16: round to nearest even, overflow to inf, subnormals kept (numpy astype(float16)).  U16: q = rint(d / scale)
 *                        in float32; NaN, +-inf and d <= 0 give 0; q > 65535 gives 65535.
 *   la3d_unpack_depth16  planes stored W_in pixels wide -> out dev f32 [P][H][W], the first W <= W_in columns, by the value rule above. */
#define LA3D_DTYPE_U16 3
#define LA3D_DEPTH_ZERO_IS_HOLE 1
typedef struct la3d_depth16 {
  int32_t struct_size;      /* sizeof(la3d_depth16) of the caller */
  int32_t dtype;            /* LA3D_DTYPE_F16 | LA3D_DTYPE_U16 */
  const void* planes;       /* device, 2-byte aligned; plane of instance n = image_index[n] or n */
  int64_t plane_stride;     /* ELEMENTS between planes, >= H*W; 0 = one shared plane */
  float scale;              /* U16: metres per unit, finite and > 0; F16: ignored */
  int32_t flags;            /* U16: LA3D_DEPTH_ZERO_IS_HOLE or 0; F16: must be 0 */
} la3d_depth16;
int la3d_fit_instances_depth16(const la3d_fit_args* args, const la3d_depth16* depth, const uint32_t* mask_bits,
                               int64_t bits_plane_stride, int32_t bits_flags);
int la3d_pack_depth16(const float* depth, int64_t plane_stride, int P, int H, int W, int W_out, int dtype, float scale, void* out,
                      int64_t out_plane_stride, void* stream);
int la3d_unpack_depth16(const la3d_depth16* src, int P, int H, int W_in, int W, float* out, void* stream);

/* ---- images of different sizes in one call ---------------------------------------------------------------------------
 * Every entry above takes ONE (H, W) per call; a COCO shard comes in hundreds of frame sizes.  la3d_fit_instances_frames fits
 * instances of images of DIFFERENT sizes in one launch: the depth planes lie in one buffer, each at its own offset and pitch, and a
 * device-resident table says where - one la3d_frame row per IMAGE:
 *   depth_offset  ELEMENTS of the depth buffer from its base to the image's plane, >= 0 and a multiple of 4: floats from
 *                 args->depth for la3d_fit_instances_frames (16-byte aligned planes), 16-bit words from depth->planes for
 *                 la3d_fit_instances_frames_depth16 (8-byte aligned planes)
 *   H, W          rows, and pixels per row IN MEMORY (the pitch), W % 32 == 0
 *   frame_width   image columns, 0 < frame_width <= W; the columns beyond are padding (what la3d_fit_args::frame_width says for a
 *                 uniform call, here per image)
 *   reserved      0
 * args: the block of la3d_fit_instances_ex, where
 *   - H, W are BOUNDS: every frame has H <= args->H and W <= args->W.  They size the kernel's LDS and the workspace
 *     (la3d_fit_workspace_bytes(args) stays the sizing call); they need not be multiples of anything, H * roundup32(W) <= 1048576;
 *   - image_index is REQUIRED: instance n belongs to frame row image_index[n] (and, as ever, to K + image_index[n] * k_stride);
 *   - depth must be 16-byte aligned; depth_plane_stride and frame_width of the block must be 0;
 *   - image_width / image_height are ignored: proj clamps to the instance's own frame_width x H;
 *   - run lengths are column-major over the instance's own (H, frame_width); polygon sides are clipped to the instance's own
 *     frame_width x H; the fused filter takes H and the right and bottom borders from the instance's frame;
 *   - masks: rle_counts (+ rle_offsets) or poly_xy (+ ring_offsets, inst_rings) - the annotation formats.  mask (u8 planes) and
 *     bit planes: LA3D_ERR_UNSUPPORTED (bit planes - and with them label maps - have an entry of their own:
 *     la3d_fit_instances_frames_bits, below).  method = LA3D_METHOD_CONVEX_HULL: LA3D_ERR_UNSUPPORTED in this first form;
 *   - ground, sample_idx (reference-subsample mode), filter_* + stats, proj, aux, area_hint, opt_launch_order, stream mean what they
 *     mean in la3d_fit_instances_ex.  The call runs on the instance engine (opt_engine pins give way, as for bit planes), in its
 *     tiled form.  The size-balanced launch order runs when area_hint is given (same batch range as elsewhere); without a hint
 *     workgroup b fits instance xcd_remap(b) - no estimate pass.  Records never depend on either.
 * frames: DEVICE pointer to P rows.  The library never synchronises, so a row that breaks the contract cannot fail the call: every
 * instance whose image_index lies outside [0, P), or whose frame row has a pitch that is not a multiple of 32, a negative or
 * misaligned depth_offset, H or W outside (0, bound], or frame_width outside (0, W], gets LA3D_BOX_UNSUPPORTED and a NaN record
 * (aux = NaN, 0, NaN, NaN; stats row untouched), decided in the kernel before any address is formed from the row; every other
 * instance of the call is fitted as if the broken row were not there.  What a conforming row addresses - H * W floats from
 * depth_offset on - must lie inside the caller's buffer: that the library cannot check.
 * Covered frames: EVERY frame inside the contract is fitted, small ones included (a frame of fewer than 64 tiles of 32 x 8 pixels,
 * the floor of the uniform entry's tiled form, is fitted too: the call's LDS is sized for at least 64 tiles whatever the bounds).
 * A call whose bounds exceed what the tiled form holds (H > 2040, W > 8160, or - subsample mode - a bit image + rank prefix beyond
 * one workgroup's LDS) returns LA3D_ERR_UNSUPPORTED as a whole.
 *
 * la3d_fit_instances_frames_depth16(args, depth, frames, P): the same call on 16-bit depth planes ("16-bit depth planes" above) - a
 * shard of sensor or network depth in many frame sizes, fitted where it lies: no float32 copy is made or read.  args and frames mean
 * what they mean in la3d_fit_instances_frames, depth what it means in la3d_fit_instances_depth16, except:
 *   - args->depth must be NULL and args->depth_plane_stride 0; depth->plane_stride must be 0 (the frame table says where every plane
 *     lies); depth->planes is the base of the ragged buffer and must be 8-byte aligned;
 *   - la3d_frame::depth_offset counts 16-BIT ELEMENTS from depth->planes; a multiple of 4 is then an 8-byte aligned plane, which is what
 *     the 16-bit vector forms need.  The on-device contract check is the same one (a depth_offset of 2 - 4 bytes - is refused with
 *     LA3D_BOX_UNSUPPORTED like any other misaligned row); a conforming row addresses H * W 16-bit words from depth_offset on;
 *   - the value rules are those of the 16-bit planes, unchanged: exact float16, ONE rounded float32(x) * scale, LA3D_DEPTH_ZERO_IS_HOLE.
 *     A call gives the records la3d_fit_instances_frames gives on the up-converted planes in the same layout, bit for bit.
 * Refused before any launch (LA3D_ERR_ARG / LA3D_ERR_UNSUPPORTED) is what either parent entry refuses: a bad block or la3d_depth16
 * (struct_size, dtype, scale, flags), a non-zero plane_stride, a misaligned base, u8 or bit-plane masks, LA3D_METHOD_CONVEX_HULL, a
 * missing image_index, a non-zero depth_plane_stride or frame_width in the block, bounds beyond the tiled form.  Workspace:
 * la3d_fit_workspace_bytes(args).
 *
 * la3d_fit_instances_frames_bits(args, depth16, frames, P, mask_bits, bits_offsets, bits_flags): the same call with the masks given as
 * bit planes ("masks as bit planes" above), one plane per instance, each as large as its OWN frame - what a panoptic dataset needs: one
 * label map per image (la3d_pack_label_bits_frames below makes the planes) and hundreds of frame sizes.
 *   - args, frames and P mean what they mean in la3d_fit_instances_frames (H, W are bounds; image_index is required;
 *     depth_plane_stride and frame_width of the block must be 0; proj clamps to the instance's own frame; the fused filter takes its
 *     borders from the instance's frame).  depth16 == NULL: float32 planes in args->depth, 16-byte aligned.  depth16 != NULL: the rules
 *     of la3d_fit_instances_frames_depth16 - args->depth NULL, plane_stride 0, an 8-byte aligned base, depth_offset in 16-bit elements;
 *   - args->mask, rle_counts and poly_xy must be NULL (LA3D_ERR_ARG): the masks are the bit planes;
 *   - the plane of instance n starts bits_offsets[n] words behind mask_bits (bits_offsets: DEVICE i64 [B]) and holds the
 *     H_f * W_f / 32 words of the frame of instance n, W_f being the pitch - a multiple of 32, so rows are whole words -, in the bit
 *     layout of la3d_fit_instances_bits.  The bits of columns >= frame_width MUST be zero (la3d_pack_label_bits_frames guarantees it).
 *     mask_bits must be 16-byte aligned - checked before any launch: LA3D_ERR_ARG -, and every bits_offsets[n] >= 0 and a multiple of
 *     4: every plane then streams into LDS in 16-byte groups.  Planes may repeat, overlap or lie in any order;
 *   - the offsets are checked ON THE DEVICE, next to the frame row and by the same rule: an instance whose offset is negative or not a
 *     multiple of 4 gets LA3D_BOX_UNSUPPORTED and the NaN record / aux / proj a broken frame row gives, decided before any address is
 *     formed from the offset; the call and every other instance are unaffected.  An instance whose frame row is broken is refused
 *     before its offset is even loaded.  What a conforming offset addresses must lie inside the caller's buffer;
 *   - ground, sample_idx (reference-subsample mode), filter_* + stats, proj, aux, area_hint, opt_launch_order and stream mean what they
 *     mean in la3d_fit_instances_frames; the height rule of the fused filter comes from bits_flags (LA3D_BITS_HEIGHT_ROWS /
 *     LA3D_BITS_HEIGHT_SPAN; other bits: LA3D_ERR_ARG).  The size-balanced launch order runs only with area_hint, as there;
 *   - method = LA3D_METHOD_CONVEX_HULL: LA3D_ERR_UNSUPPORTED, as for every frames call.  Everything else either parent entry refuses
 *     before a launch is refused here.  Workspace: la3d_fit_workspace_bytes(args).
 * The records are those of la3d_fit_instances_frames on run lengths of the same masks, bit for bit: the same kernel on the same bit
 * image in LDS.
 *
 * la3d_pack_label_bits_frames: la3d_pack_label_bits ("masks as label maps" above) for label maps of DIFFERENT sizes in one buffer.
 *   labels: dev, 16-byte aligned; image p lies frames[p].depth_offset ELEMENTS (pixels for RGB8) behind it, its rows frames[p].W
 *     elements apart, frames[p].H rows of frames[p].frame_width image columns - a label buffer packed the way the depth is packed has
 *     exactly the depth's table: ONE table serves this packer and the fit.  H, W: the bounds of the table (as in the fit);
 *   inst_offsets dev [P+1], inst_label dev [B], area dev [B] | NULL: as in la3d_pack_label_bits;
 *   bits, bits_offsets dev i64 [B]: the plane of row b is written at bits + bits_offsets[b]: the H_f * W_f / 32 words of its image's
 *     frame, every word of them and nothing else.
 * VALUE: the rule of la3d_pack_label_bits (compared as int32; an id outside the dtype: an all-zero plane; repeated rows each get their
 *   plane), and: bits of columns >= frame_width are ZERO WHATEVER THE PADDING ELEMENTS HOLD (RGB8: they are not even read) - id 0
 *   asked of a zero-padded map marks image pixels only.
 * Rows of an image whose frame row breaks the la3d_frame contract (the check of the fit, made on the device), and rows whose
 *   bits_offsets entry is negative or not a multiple of 4, are NOT written and nothing is read through either: exactly the instances
 *   the fit then refuses.  Their area stays 0.
 * U8 / U16 / I32 planes are read in 16-byte groups where they are 16-byte aligned (every I32 plane; U8 / U16 planes at offsets that are
 *   multiples of 16 / 8 elements - what back-to-back packing gives) and in 4-byte loads otherwise; RGB8 byte by byte.
 * LA3D_ERR_ARG: an unknown dtype, negative sizes, bounds beyond H * roundup32(W) <= 2^28, misaligned or NULL pointers with work to do.
 *   B == 0 or P == 0: success, nothing is done.  The call is capturable (area is cleared by a kernel of the call).
 *
 * la3d_pack_mask_bits_frames / la3d_pack_logits_bits_frames: la3d_pack_mask_bits / la3d_pack_logits_bits ("masks as bit planes"
 * above) for B planes of DIFFERENT sizes in one launch - the (N_p, H_p, W_p) stack of u8 / boolean masks or of logits an
 * instance-segmentation network gives per image, read where it lies - into the planes la3d_fit_instances_frames_bits fits.
 *   SOURCE: instance n belongs to image image_index[n] (dev i32 [B]: the array the fit takes).  Its plane starts src_offsets[n]
 *     ELEMENTS (dev i64 [B]) behind mask / logits and has frames[p].H rows of frames[p].frame_width image columns, the rows
 *     src_pitch[n] elements apart (dev i32 [B]); src_pitch == NULL: frame_width apart - a dense (H_p, W_p) plane.  No padding to a
 *     multiple of 32 is asked of the source (only the OUTPUT has the frame's pitch frames[p].W).  The base pointer is aligned to its
 *     element; any offset >= 0 and any pitch >= frame_width is packed.  frames, P, H, W (bounds): as in the fit - ONE table serves
 *     this packer and the fit;
 *   VALUE: u8: bit = byte != 0.  Logits (LA3D_DTYPE_F32 / F16 / BF16): bit = x > threshold, compared in float32 (NaN -> 0, +inf -> 1
 *     unless threshold is +inf, -inf -> 0): the rules of la3d_pack_logits_bits;
 *   OUTPUT: exactly what la3d_pack_label_bits_frames writes - the plane of row n at bits + bits_offsets[n] (dev i64 [B]), the
 *     H_f * W_f / 32 words of its image's frame (W_f: the pitch of the table), every word of them and nothing else, the bits of
 *     columns >= frame_width zero; area[n] (dev [B] | NULL) = the popcount of the plane, cleared by a kernel of the call: the call is
 *     capturable and never synchronises.
 * Checked ON THE DEVICE, before any address is formed from the value:
 *   - a row whose image_index is outside [0, P), whose frame row breaks the la3d_frame contract (the check of the fit), or whose
 *     bits_offsets entry is negative or not a multiple of 4 is NOT written and nothing is read for it: exactly the instances the fit
 *     then refuses (LA3D_BOX_UNSUPPORTED).  Their area stays 0;
 *   - a row whose src_offsets entry is negative, or whose pitch is smaller than its frame_width, is written as an ALL-ZERO plane with
 *     area 0 and nothing is read through it: the fit cannot see the source, so such an instance comes back EMPTY (LA3D_BOX_EMPTY),
 *     never fitted to whatever the memory held before.
 * What is read of a conforming instance: only elements (v, u) with v < H_f and u < pitch, and in the last row nothing beyond the last
 *   image column - a dense plane that ends at the end of an allocation is a normal input.  Planes whose first byte and byte pitch are
 *   multiples of 16 are read in 16-byte groups, every other plane element by element.
 * LA3D_ERR_ARG before any launch: an unknown dtype, negative B or P, bounds <= 0 or beyond H * roundup32(W) <= 2^28,
 *   B * ceil(H * roundup32(W) / 8192) >= 2^31, NULL or misaligned pointers with work to do.  B == 0 or P == 0: success, nothing is done. */
typedef struct la3d_frame {      /* one row per IMAGE, device-resident */
  int64_t depth_offset;          /* elements from the base of the depth buffer to this image's plane, % 4 == 0: floats from args->depth
                                    (la3d_fit_instances_frames), 16-bit words from depth->planes (la3d_fit_instances_frames_depth16) */
  int32_t H, W;                  /* rows; pixels per row IN MEMORY (the pitch), W % 32 == 0 */
  int32_t frame_width;           /* image columns, 0 < frame_width <= W; columns beyond are padding */
  int32_t reserved;              /* 0 */
} la3d_frame;
int la3d_fit_instances_frames(const la3d_fit_args* args, const la3d_frame* frames, int32_t P);
int la3d_fit_instances_frames_depth16(const la3d_fit_args* args, const la3d_depth16* depth, const la3d_frame* frames, int32_t P);
int la3d_fit_instances_frames_bits(const la3d_fit_args* args, const la3d_depth16* depth16 /* NULL: float32 planes in args->depth */,
                                   const la3d_frame* frames, int32_t P,
                                   const uint32_t* mask_bits, const int64_t* bits_offsets /* dev [B] */, int32_t bits_flags);
int la3d_pack_label_bits_frames(const void* labels, int dtype, const la3d_frame* frames, int32_t P, int H, int W /* bounds */,
                                const int32_t* inst_offsets /* dev [P+1] */, const int32_t* inst_label /* dev [B] */, int B,
                                uint32_t* bits, const int64_t* bits_offsets /* dev [B] */, int32_t* area /* dev [B] or NULL */, void* stream);
int la3d_pack_mask_bits_frames(const uint8_t* mask, const la3d_frame* frames, int32_t P, int H, int W /* bounds */,
                               const int32_t* image_index /* dev [B] */, const int64_t* src_offsets /* dev [B], ELEMENTS from mask */,
                               const int32_t* src_pitch /* dev [B] ELEMENTS between rows, or NULL = frame_width of the row's image */,
                               int B, uint32_t* bits, const int64_t* bits_offsets /* dev [B] */, int32_t* area /* dev [B] or NULL */,
                               void* stream);
int la3d_pack_logits_bits_frames(const void* logits, int dtype /* LA3D_DTYPE_F32 | F16 | BF16 */, float threshold,
                                 const la3d_frame* frames, int32_t P, int H, int W /* bounds */,
                                 const int32_t* image_index /* dev [B] */, const int64_t* src_offsets /* dev [B], ELEMENTS from logits */,
                                 const int32_t* src_pitch /* dev [B] ELEMENTS between rows, or NULL = frame_width of the row's image */,
                                 int B, uint32_t* bits, const int64_t* bits_offsets /* dev [B] */, int32_t* area /* dev [B] or NULL */,
                                 void* stream);

/* create_boolean_mask_from_polygon for a batch: polygon parts -> u8 planes mask_out dev [B][H*W] (0/1). */
int la3d_poly_decode(const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, int B, int H, int W,
                     uint8_t* mask_out, void* stream);

/* The four filter quantities of la3d_mask_stats for polygon annotations, rasterised in LDS (no plane is written):
 * replaces create_boolean_mask_from_polygon + get_maximum_height + analyze_mask (src/util.py:291-335, :371-375). */
int la3d_mask_stats_poly(const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, int B, int H, int W,
                         int boundary, int32_t* stats, void* stream);

/* ---- annotations as bit planes -----------------------------------------------------------------------------------------
 * la3d_rle_decode / la3d_poly_decode with the bit image kept as the output: COCO run lengths and polygon parts -> the planes of
 * "masks as bit planes" (38 400 B per 640x480 instance instead of the 307 200 B of a u8 plane), for every consumer of planes that
 * is not the fit itself (the fit decodes annotations inside its own kernel): la3d_gather_instance_points, la3d_mask_stats_bits,
 * la3d_unpack_mask_bits, and la3d_fit_instances_bits / la3d_fit_instances_frames_bits for planes that stay resident.  One workgroup
 * per instance decodes into LDS and streams the words out; the call never synchronises and is capturable (one kernel, no clear).
 *
 * la3d_pack_rle_bits / la3d_pack_poly_bits (one frame size): the annotation arrays as la3d_rle_decode / la3d_poly_decode take them
 *   (counts + offsets [B+1]: column-major runs over (H, W), zeros first; poly_xy + ring_offsets + inst_rings [B+1]).
 *   Output: B planes in exactly the format of la3d_pack_mask_bits - la3d_mask_bits_words(H, W_out) words each, bits_plane_stride
 *   words apart, rows padded from W to W_out with zero bits; every word of every plane is written and nothing else.  W_out is W (any
 *   width: the decoders' general routes) or a multiple of 32 >= W (the next one is what the tiled forms of the fit want).  A
 *   16-byte aligned base with bits_plane_stride % 4 == 0 is written in 16-byte groups, anything else word by word.
 *   area: dev [B] or NULL - the popcount of each plane as written (what area_hint wants), stored by the plane's own workgroup.
 *   LA3D_ERR_ARG: negative B, H, W <= 0, W_out < W, a W_out != W that is no multiple of 32, bits_plane_stride <
 *   la3d_mask_bits_words(H, W_out), NULL or misaligned (4 bytes) pointers with work to do.  H*W_out > 1048576 (the bit image lives
 *   in LDS): LA3D_ERR_UNSUPPORTED.  B == 0: success, nothing is launched.
 * la3d_pack_rle_bits_frames / la3d_pack_poly_bits_frames (images of different sizes): instance n belongs to image image_index[n]
 *   (dev i32 [B]); its runs are column-major over its own (H_f, frame_width), its polygon sides are clipped to its own frame_width x
 *   H_f - the rules of la3d_fit_instances_frames.  frames, P, H, W (bounds): as in the fit - ONE table serves packer and fit.
 *   Output: the contract of la3d_pack_mask_bits_frames - the plane of row n at bits + bits_offsets[n] (dev i64 [B]), the H_f * W_f / 32
 *   words of its image's frame, every word of them and nothing else, the bits of columns >= frame_width zero; bits 16-byte aligned
 *   (LA3D_ERR_ARG otherwise).  Checked ON THE DEVICE, each before an address is formed from the value, in this order:
 *   image_index[n] in [0, P); the frame row (the check of the fit); bits_offsets[n] >= 0 and a multiple of 4.  A refused row writes
 *   no plane word and gets area 0: exactly the instances the fit then answers with LA3D_BOX_UNSUPPORTED.
 *   LA3D_ERR_ARG: negative B or P, bounds <= 0, NULL or misaligned pointers with work to do; bounds beyond H * roundup32(W) <=
 *   1048576: LA3D_ERR_UNSUPPORTED.  B == 0: success, nothing is launched.
 * HOSTILE RUN LISTS.  Whatever a run list holds, only the words of the instance's own plane are written (the decode goes to LDS, the
 *   copy covers exactly the plane): a negative count is a run of length 0, runs past H * frame_width are cut, an offsets pair that
 *   goes backwards gives an empty plane.  What offsets / ring_offsets / inst_rings ADDRESS must lie inside the caller's arrays. */
int la3d_pack_rle_bits(const int32_t* counts, const int64_t* offsets, int B, int H, int W, int W_out, uint32_t* bits,
                       int64_t bits_plane_stride, int32_t* area /* dev [B] or NULL */, void* stream);
int la3d_pack_poly_bits(const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, int B, int H, int W, int W_out,
                        uint32_t* bits, int64_t bits_plane_stride, int32_t* area /* dev [B] or NULL */, void* stream);
int la3d_pack_rle_bits_frames(const int32_t* counts, const int64_t* offsets, const la3d_frame* frames, int32_t P, int H, int W /* bounds */,
                              const int32_t* image_index /* dev [B] */, int B, uint32_t* bits, const int64_t* bits_offsets /* dev [B] */,
                              int32_t* area /* dev [B] or NULL */, void* stream);
int la3d_pack_poly_bits_frames(const int32_t* poly_xy, const int64_t* ring_offsets, const int64_t* inst_rings, const la3d_frame* frames,
                               int32_t P, int H, int W /* bounds */, const int32_t* image_index /* dev [B] */, int B, uint32_t* bits,
                               const int64_t* bits_offsets /* dev [B] */, int32_t* area /* dev [B] or NULL */, void* stream);

/* ---- bit planes as run lengths ------------------------------------------------------------------------------------------
 * The way back out of a plane: binary_mask_to_rle for a batch (reference src/download_coconut.py:167-175) - the planes of "masks as
 * bit planes", whatever packer made them, become COCO run lengths on the device: a few hundred bytes per instance, the fastest source
 * of the fit (la3d_fit_instances_rle), what the sharded entries ship and what the annotation JSON stores.  All B run lists are packed
 * into ONE counts array with an offsets array - exactly what la3d_fit_instances_rle, la3d_rle_decode, la3d_mask_stats_rle and
 * la3d_pack_rle_bits take.  Two stages on the caller's stream; neither synchronises, so the chain can be captured into a HIP graph:
 *   la3d_rle_encode_offsets(args)  runs[n] (i32 [B]) = the number of counts of instance n's run list; offsets (i64 [B+1]) = the
 *       exclusive prefix of runs, scanned on the device, deterministic, any B.  Per column the number of transitions and the row of
 *       the last one stay in `workspace` for the second stage.  B == 0: offsets[0] = 0, nothing else is launched.
 *   la3d_rle_encode(args)          counts[offsets[n] .. offsets[n+1]) (i32) = the run list of instance n.  The place of a count is the
 *       rank of the transition that ends it, from prefixes over the columns - never from atomics.
 * Both take the SAME block (the second stage reads offsets and workspace as the first left them; counts, status and capacity are not
 * read by the first stage, runs not by the second).
 * VALUE.  The runs of the (H, frame_width) image in COLUMN-major order (flat index u * H + v), alternating zeros and ones, zeros
 *   first: a leading 0 when pixel (0, 0) is set; an all-zero plane gives [H * frame_width], an all-one plane [0, H * frame_width];
 *   runs = transitions + 1 + bit(0, 0).  The list is the reference's, count for count.
 * WHAT IS READ OF A PLANE.  Only bits (v, u) with v < H and u < frame_width: the pad bits of rows stored W > frame_width wide and
 *   the bits of the last word past H * W are never read as mask, whatever they hold.
 * FORMS.  frames == NULL: B planes of ONE H x W in the layout of la3d_pack_mask_bits (W = pixels per row in memory; frame_width
 *   0 = W, else the image columns), bits_plane_stride words apart (0 = the words of a plane), 4-byte aligned; a 16-byte aligned base
 *   with a stride that is a multiple of 4 is streamed in 16-byte groups, anything else word by word.  frames != NULL selects the
 *   FRAMES form (one pair of entries serves both): the plane of row n at mask_bits + bits_offsets[n] (dev i64 [B]), its geometry
 *   frames[image_index[n]] - the table and the planes of la3d_fit_instances_frames_bits; H, W are bounds, image_index is required,
 *   frame_width and bits_plane_stride must be 0, mask_bits 16-byte aligned.  Checked ON THE DEVICE, each before an address is formed
 *   from the value, in the order of the packers: image_index[n] in [0, P); the frame row (the check of the fit); bits_offsets[n] >= 0
 *   and a multiple of 4.  A refused row gets runs 0, nothing is read or written for it, and status 5 (LA3D_BOX_UNSUPPORTED).
 * STATUS (i32 [B], written by the second stage).  The second stage never writes outside counts[offsets[n] .. offsets[n+1]) of its
 *   own instance, whatever the planes hold: LA3D_RLE_NO_ROOM - the range does not lie within [0, capacity]: nothing of the instance is
 *   written; LA3D_RLE_MISMATCH - the plane's run count differs from the range length, or a column from what the first stage left in
 *   the workspace (the planes changed between the two calls): the range is filled only as far as it reaches, with values that mean
 *   nothing.
 * workspace: la3d_rle_encode_workspace_bytes(B, H, W) bytes (host, no device; 0 for B, H or W <= 0), 8-byte aligned; ONE workspace
 *   serves one pair of calls at a time.
 * LA3D_ERR_ARG before any launch: a bad struct_size, negative sizes, strides or capacity, frame_width outside [0, W], an empty frame
 *   with B > 0, bits_plane_stride below the words of a plane, bits_offsets without frames, frames without image_index, NULL or
 *   misaligned pointers with work to do (offsets always; counts may be NULL with capacity 0).  H * W (frames: H * roundup32(W))
 *   > 1048576: LA3D_ERR_UNSUPPORTED - the bit image lives in LDS, as for every consumer of planes. */
#define LA3D_RLE_OK 0
#define LA3D_RLE_NO_ROOM 1
#define LA3D_RLE_MISMATCH 2
typedef struct la3d_rle_encode_args {
  int32_t struct_size;                                   /* sizeof(la3d_rle_encode_args) of the caller */
  int32_t B, H, W;
  int32_t frame_width;                                   /* 0 = W */
  int32_t P;                                             /* rows of frames */
  const uint32_t* mask_bits; int64_t bits_plane_stride;  /* bit planes; words between planes, 0 = the words of a plane */
  const la3d_frame* frames;                              /* dev [P] | NULL: the frames form */
  const int32_t* image_index;                            /* dev [B], frames form */
  const int64_t* bits_offsets;                           /* dev [B], frames form */
  int32_t* runs;                                         /* dev [B]: first stage */
  int64_t* offsets;                                      /* dev [B+1]: written by the first stage, read by the second */
  int32_t* counts;                                       /* dev [capacity]: second stage */
  int32_t* status;                                       /* dev [B]: second stage */
  int64_t capacity;                                      /* counts the array holds */
  void* workspace; void* stream;
} la3d_rle_encode_args;
size_t la3d_rle_encode_workspace_bytes(int B, int H, int W);
int la3d_rle_encode_offsets(const la3d_rle_encode_args* args);
int la3d_rle_encode(const la3d_rle_encode_args* args);

/* ---- crop-space masks as bit planes ------------------------------------------------------------------------------------
 * restore_mask_from_crop for a batch (reference src/util.py:171-214; the box stage calls it per object, src/batch_scripts/
 * whole.py:72-105): the S x S mask of a crop - or the alpha channel of its RGBA image, thresholded - resized by nearest index to
 * side x side pixels and pasted, clipped, into a full frame; written as the planes of "masks as bit planes", never as a u8 plane.
 *
 * SOURCE.  Byte (y, x) of crop n lies at crops + n*crop_stride + y*row_pitch + x*pixel_step (all in BYTES): a dense u8 / bool mask is
 *   (S*S, S, 1); the alpha of dense RGBA crops is crops = base + 3 with (4*S*S, 4*S, 4).  bit = byte > threshold (0 for masks, 127
 *   for alpha: whole.py:83).
 * place dev i32 [B][4], 4-byte aligned: x1, y1, side, 0 (the fourth is not read).  The HOST computes them, in float64 as the
 *   reference does: side = int(S / scale_factor) (truncated), x1 = int(round(offset_x)), y1 = int(round(offset_y)) with Python's
 *   round (half to even).
 * VALUE.  Bit (v, u) of plane n is 0 unless x1 <= u < x1 + side, y1 <= v < y1 + side, u < W and v < H; there it is
 *   crop[sy][sx] > threshold with sx = min(floor((u - x1) * ifx), S - 1), sy likewise, ifx = 1.0 / ((double)side / (double)S) - one
 *   float64 multiply, then floor: the index rule of OpenCV's INTER_NEAREST resize (resizeNN, inv_scale = dsize / ssize).
 * TWO CASES DIFFER FROM THE REFERENCE, both give an all-zero plane and area 0 (LA3D_BOX_EMPTY in the fit), never an error of the call:
 *   side <= 0 (cv2.resize raises there), and a placement wholly outside the frame (the reference's slice assignment raises a
 *   broadcast ValueError in most such cases and pastes nothing in the rest).
 * ADDRESSING.  place is read on the device and checked before an address is formed from it: side must lie in (0, 2^20] - a larger
 *   side is treated like side <= 0: an all-zero plane -, x1 and y1 may be any int32 (the differences are taken in 64 bits).  A row with
 *   an empty plane reads nothing from crops, and whatever place holds only bytes (y, x) with 0 <= y, x < S of the row's OWN crop are
 *   addressed.
 * la3d_pack_crop_bits (one frame size): the output contract of la3d_pack_rle_bits - B planes of la3d_mask_bits_words(H, W_out) words,
 *   bits_plane_stride words apart, rows padded from W to W_out (W, or a multiple of 32 >= W) with zero bits; every word of every plane
 *   is written and nothing else.  la3d_pack_crop_bits_frames (images of different sizes): the contract of la3d_pack_rle_bits_frames -
 *   the plane of row n at bits + bits_offsets[n], the words of its image's frame, bits 16-byte aligned; checked on the device in the
 *   same order (image_index[n], the frame row, bits_offsets[n]); a refused row writes no word and gets area 0.
 *   area: dev [B] or NULL - the popcount of each plane as written; cleared by a kernel of the call on `stream` and accumulated with
 *   one integer atomic per wave.  One packing kernel (plus that clear), no synchronisation: the call is capturable.
 * LA3D_ERR_ARG / LA3D_ERR_UNSUPPORTED: as for la3d_pack_rle_bits / la3d_pack_rle_bits_frames (H*W_out, or the bounds' H *
 *   roundup32(W), beyond 1048576: LA3D_ERR_UNSUPPORTED - what the consumers of planes take); and LA3D_ERR_ARG for S <= 0,
 *   pixel_step < 1, row_pitch < S*pixel_step, threshold outside [0, 255], crop_stride smaller than a crop ((S-1)*row_pitch +
 *   (S-1)*pixel_step + 1 bytes), a misaligned place - these are checked first, for B == 0 too.  B == 0 otherwise: success, nothing is
 *   launched. */
int la3d_pack_crop_bits(const uint8_t* crops, int64_t crop_stride /* bytes between crops */, int32_t row_pitch /* bytes */,
                        int32_t pixel_step /* bytes between pixels */, int S, int threshold /* bit = byte > threshold */,
                        const int32_t* place /* dev [B][4]: x1, y1, side, 0 */, int B, int H, int W, int W_out, uint32_t* bits,
                        int64_t bits_plane_stride, int32_t* area /* dev [B] or NULL */, void* stream);
int la3d_pack_crop_bits_frames(const uint8_t* crops, int64_t crop_stride, int32_t row_pitch, int32_t pixel_step, int S, int threshold,
                               const int32_t* place /* dev [B][4] */, const la3d_frame* frames, int32_t P, int H, int W /* bounds */,
                               const int32_t* image_index /* dev [B] */, int B, uint32_t* bits, const int64_t* bits_offsets /* dev [B] */,
                               int32_t* area /* dev [B] or NULL */, void* stream);

/* ---- morphology on bit planes ------------------------------------------------------------------------------------------
 * The mask step between the annotations and the crops (reference src/batch_scripts/get_crops_enhanced.py:68-99): each instance mask
 * is resized x4 with nearest neighbour, opened with scipy.ndimage.binary_opening(mask, np.ones((7, 7))), dropped when fewer than 6400
 * pixels survive, and the cv2.boundingRect of what is left gives the (offset_x, offset_y, scale_factor) that "crop-space masks as bit
 * planes" takes.  la3d_open_bits does the upscale, the opening, the area and the rectangle for a batch of planes in one pass; at
 * upscale 1 it strips speckle and hairlines from network masks before a fit.
 * VALUE, per plane.  M = the H x frame_width mask; U = its nearest-neighbour upscale by s = upscale, U[v, u] = M[v / s, u / s] (integer
 *   division); out = binary_opening(U, ones((k, k))) as SciPy defines it: an erosion, then a dilation, both with border_value = 0 and
 *   origin 0 - pixels outside the image count as unset.  k is odd, 1 .. 31; k = 1 is the identity.  upscale is 1, 2 or 4: for these
 *   factors 1 / s is exact in binary floating point, so EVERY nearest rule - OpenCV's floor(x * (1 / s)) included - gives u / s; that
 *   is why 3 is not offered.  (The opening is pinned to SciPy bit for bit, tests/golden/g19_opening.npz; the nearest rule and the
 *   rectangle convention are restated, parity unpinned until OpenCV is at hand.)
 * INPUT.  B planes of "masks as bit planes", stored W pixels wide (rows need not start on a word when W % 32 != 0), bits_plane_stride
 *   words apart.  Columns at and beyond frame_width are zero by the format's contract and are masked here anyway; the bits of the
 *   last word past H * W are never read as mask.
 * OUTPUT.  out_bits (NULL: statistics only): planes of s * H rows stored W_out >= s * frame_width pixels wide, out_plane_stride words
 *   apart, same format.  Only the la3d_mask_bits_words(s * H, W_out) words of each plane are written; the pad columns and the tail
 *   bits of the last word are zero.  A 16-byte aligned base with W_out % 128 == 0 and a stride that is a multiple of 4 is written in
 *   16-byte stores, W_out % 32 == 0 word by word, anything else through a general form that gathers each word from the rows crossing it.
 * STATISTICS.  stats[b] (NULL: none) = {area, x, y, w, h} of the output plane in output pixels: x, y, w, h as cv2.boundingRect gives
 *   them for a binary image - the tight box of the set pixels -, 0, 0, 0, 0 for an empty plane.  k = 1, upscale = 1, out_bits = NULL
 *   is a pure area-and-rectangle pass over planes.
 * workspace: la3d_open_bits_workspace_bytes(B, H, upscale) bytes (host, no device; 0 for B, H <= 0), 4-byte aligned; needed with
 *   stats (one record per band of output rows, reduced per instance by a second kernel: two stages, no atomics).  The call takes no
 *   host synchronisation and can be captured into a HIP graph.
 * Refused before any launch - LA3D_ERR_ARG: B < 0, H, W <= 0; k even or outside 1 .. 31; upscale not 1, 2 or 4; frame_width outside
 *   (0, W]; out_bits and stats both NULL; W_out < s * frame_width (with out_bits; without it W_out is not read); with B > 0: bits NULL, workspace NULL with stats, a pointer that
 *   is not 4-byte aligned, a stride shorter than its plane, or word ranges [bits, bits + B * bits_plane_stride) and [out_bits,
 *   out_bits + B * out_plane_stride) that overlap (neighbouring bands read each other's halo: the call cannot work in place).
 *   LA3D_ERR_UNSUPPORTED: s * frame_width > 8192 (a band of rows lives in LDS) or s * H * W_out > 2^28.  B == 0 returns 0, no launch. */
size_t la3d_open_bits_workspace_bytes(int B, int H, int upscale);
int la3d_open_bits(const uint32_t* bits, int64_t bits_plane_stride, int B, int H, int W, int frame_width, int k, int upscale,
                   uint32_t* out_bits /* NULL: statistics only */, int64_t out_plane_stride, int W_out,
                   int32_t* stats /* dev [B][5] or NULL */, void* workspace, void* stream);
/* la3d_open_bits_frames: the same VALUE and STATISTICS for the planes of images of DIFFERENT sizes in one call ("images of different
 * sizes in one call": the la3d_frame table, P rows, and its bounds H, W - the largest rows and the largest pitch).  One k and one
 * upscale per call; the structuring element is a square.
 * INPUT.  Row n belongs to image image_index[n]; its plane lies at bits + bits_offsets[n] and holds the H_f * W_f / 32 words of that
 *   image's frame row (H_f rows, pitch W_f - a multiple of 32 -, frame_width fw_f image columns).  Columns at and beyond fw_f count as
 *   zero whatever the plane holds, and so does everything outside rows [0, H_f).  bits_words: the words of the buffer at bits.
 * OUTPUT.  out_bits (NULL: statistics only): the plane of row n at out_bits + out_offsets[n], in the layout the frame table of an
 *   image of size (s * H_f, s * fw_f) has: s * H_f rows, pitch roundup32(s * fw_f), frame_width s * fw_f.  A conforming row writes
 *   exactly the s * H_f * roundup32(s * fw_f) / 32 words of its plane - the bits of the padding columns zero - and nothing else.  The
 *   planes must not overlap each other; out_words: the words of the buffer at out_bits.
 * CHECKED ON THE DEVICE, per row, every value wave-uniform and before an address is formed from it, in this order: image_index[n]
 *   inside [0, P); the frame row against the la3d_frame contract and the bounds (the check of the fit); bits_offsets[n] >= 0 and a
 *   multiple of 4; out_offsets[n] likewise (with out_bits); then that the planes end inside their buffers: bits_offsets[n] + words
 *   <= bits_words and out_offsets[n] + words <= out_words.  A refused row reads nothing, writes no plane word and gets the statistics
 *   row -1, 0, 0, 0, 0: area -1 tells it from an empty plane (0, 0, 0, 0, 0), and area >= min_area stays false for it.
 * workspace: la3d_open_bits_frames_workspace_bytes(B, H, upscale) bytes with H the bound (host, no device; 0 for B, H <= 0), 4-byte
 *   aligned, needed with stats.  Nothing depends on what it held before: only band records this call wrote are read.  Two kernels
 *   (the bands of the bounds for every row - a row with fewer bands leaves the rest idle -, then one wave per row for the
 *   statistics), no atomics, no host synchronisation: the call can be captured into a HIP graph.
 * PARITY.  The opening is pinned to SciPy bit for bit (tests/golden/g19_opening.npz); the nearest rule and the rectangle convention
 *   are restated, parity unpinned, as for la3d_open_bits.
 * Refused before any launch, for B == 0 too - LA3D_ERR_ARG: B, P < 0, bounds H, W <= 0; k even or outside 1 .. 31; upscale not 1, 2
 *   or 4; out_bits and stats both NULL; bits_words < 0, out_words < 0 with out_bits; bits or out_bits not 16-byte aligned;
 *   bits_offsets, out_offsets or frames not 8-byte aligned; stats, workspace or image_index not 4-byte aligned; the word ranges
 *   [bits, bits + bits_words) and [out_bits, out_bits + out_words) overlapping (the call cannot work in place); and with B > 0: bits,
 *   bits_offsets, image_index or - with P > 0 - frames NULL, out_offsets NULL with out_bits, workspace NULL with stats.
 *   LA3D_ERR_UNSUPPORTED: upscale * W > 8192, upscale * H * roundup32(upscale * W) > 2^28, B * bands > 2^31 - 1.
 *   B == 0 returns 0 with nothing launched.  P == 0 with B > 0: every row is refused - no plane kernel runs, the statistics rows (if
 *   asked for) are -1, 0, 0, 0, 0. */
size_t la3d_open_bits_frames_workspace_bytes(int B, int H /* bound */, int upscale);
int la3d_open_bits_frames(const uint32_t* bits, int64_t bits_words, const int64_t* bits_offsets /* dev [B] */,
                          const la3d_frame* frames, int32_t P, int H, int W /* bounds of the table */,
                          const int32_t* image_index /* dev [B] */, int B, int k, int upscale,
                          uint32_t* out_bits /* NULL: statistics only */, int64_t out_words, const int64_t* out_offsets /* dev [B] */,
                          int32_t* stats /* dev [B][5] or NULL */, void* workspace, void* stream);

/* ---- connected components on bit planes --------------------------------------------------------------------------------
 * What tells a mask as it arrives from a mask worth fitting: an occluded COCO instance arrives as several polygon parts, a network
 * mask with islands far from the object, and the depth + mask fit takes every set pixel.  la3d_open_bits removes by SHAPE (it also
 * eats thin true structure and leaves any island wider than k alone); this entry removes by COMPONENT - keep the largest part, or drop
 * the parts under an area - for a batch of planes in one launch, without the unpack / device-to-host copy / scipy.ndimage.label /
 * np.bincount / pack round trip per instance.
 * VALUE, per plane (exact integers).  M = the H x frame_width image of a plane of "masks as bit planes"; columns at and beyond
 *   frame_width and bits past H * W count as zero whatever they hold.  labels, n = scipy.ndimage.label(M, structure): connectivity 8
 *   is structure = ones((3, 3)), connectivity 4 the cross (SciPy's default).  Components are numbered 1 .. n in raster order of their
 *   first pixel - that order is part of the contract.  Candidates: the components with area >= min_area.  largest = 0 keeps every
 *   candidate, largest = 1 only the candidate of greatest area, ties going to the lowest label.  The output plane is the union of
 *   the kept components, in the input's geometry (H rows, pitch W, frame_width): all la3d_mask_bits_words(H, W) words of it are
 *   written, pad columns and tail bits zero.
 * STATISTICS.  stats[b] (i32 [8]) = n_components, n_kept, area_in, area_out, x, y, w, h - the rectangle of the OUTPUT plane as
 *   cv2.boundingRect gives it for a binary image (the convention la3d_open_bits restates), 0, 0, 0, 0 for an empty output.
 * TABLE.  components[b][j] (i32 [5]) = area, x, y, w, h of the component with label j + 1, for j < min(n, max_components); the rows
 *   beyond are zero.  n_components of stats tells a truncated table from a complete one.
 * CAPACITY.  A RUN is a maximal horizontal span of set pixels within one image row; the call works on runs, never on a label per
 *   pixel, and max_runs is the caller's bound on the runs of one plane.  A plane with more runs is never labelled wrongly or partly:
 *   its stats row is -1, runs, 0, 0, 0, 0, 0, 0 with runs the count it needs (call again with that), its output plane is written as
 *   all zeros, its table rows are zero.  The other planes of the batch are not affected.
 * workspace: la3d_components_workspace_bytes(B, H, max_runs) = B * (16 * max_runs + 8 * H) bytes (host, no device; 0 for B, H or
 *   max_runs <= 0), 4-byte aligned: per run its start, its end and two words of the union-find, per row the index of its first run.
 *   Nothing depends on what it held before.  One kernel, one workgroup per plane, no host synchronisation, no allocation: the call
 *   can be captured into a HIP graph.  Deterministic: labels are ranks from prefix sums, the only atomics are integer min / max / add.
 * Refused before any launch, in this order - LA3D_ERR_ARG: a NULL block or a bad struct_size; B < 0, H, W <= 0; frame_width outside
 *   [0, W]; connectivity not 4 or 8; largest not 0 or 1; min_area < 0; max_runs < 1; max_components < 0; components without
 *   max_components > 0; out_bits, stats and components all NULL.  LA3D_ERR_UNSUPPORTED: H * W > 1048576 (what the consumers of planes
 *   take); max_runs > 524288 (a plane of 1048576 pixels has no more runs).  B == 0 then returns 0 with no launch.  With B > 0,
 *   LA3D_ERR_ARG: mask_bits or workspace NULL; a pointer that is not 4-byte aligned; a stride shorter than a plane; word ranges
 *   [mask_bits, mask_bits + B * bits_plane_stride) and [out_bits, out_bits + B * out_plane_stride) that overlap (the output is
 *   gathered from the runs of the input: the call cannot work in place). */
typedef struct la3d_components_args {
  int32_t struct_size;                                   /* sizeof(la3d_components_args) of the caller */
  int32_t B, H, W;
  int32_t frame_width;                                   /* 0 = W */
  int32_t connectivity;                                  /* 4 | 8 */
  int32_t min_area;                                      /* >= 0: components below it are dropped */
  int32_t largest;                                       /* 0: every candidate | 1: the largest candidate */
  int32_t max_runs;                                      /* runs one plane may have: 1 .. 524288 */
  int32_t max_components;                                /* rows of the table per plane */
  const uint32_t* mask_bits; int64_t bits_plane_stride;  /* bit planes; words between planes, 0 = the words of a plane */
  uint32_t* out_bits; int64_t out_plane_stride;          /* NULL: statistics only; words between planes, 0 = the words of a plane */
  int32_t* stats;                                        /* dev [B][8] or NULL */
  int32_t* components;                                   /* dev [B][max_components][5] or NULL */
  void* workspace; void* stream;
} la3d_components_args;
size_t la3d_components_workspace_bytes(int B, int H, int max_runs);
int la3d_components_bits(const la3d_components_args* args);
/* la3d_components_bits_frames: the same VALUE, STATISTICS, TABLE and CAPACITY rule for the planes of images of DIFFERENT sizes in one
 * call ("images of different sizes in one call": the la3d_frame table, P rows, and its bounds H, W - the largest rows and the largest
 * pitch).  One connectivity, min_area, largest, max_runs and max_components per call.
 * INPUT.  Row n belongs to image image_index[n]; its plane lies at bits + bits_offsets[n] and holds the H_f * W_f / 32 words of that
 *   image's frame row (H_f rows, pitch W_f - a multiple of 32 -, frame_width fw_f image columns).  Columns at and beyond fw_f count as
 *   zero whatever the plane holds.  bits_words: the words of the buffer at bits.
 * OUTPUT.  out_bits (NULL: statistics only): the plane of row n at out_bits + out_offsets[n], in the INPUT's geometry (H_f rows, pitch
 *   W_f, frame_width fw_f) - out_offsets may be the very pointer given as bits_offsets: the same layout serves a second buffer.  A
 *   conforming row writes exactly the H_f * W_f / 32 words of its plane - the bits of the padding columns zero - and nothing else.
 *   The planes must not overlap each other; out_words: the words of the buffer at out_bits.
 * CONFORMING ROWS get what la3d_components_bits gives for the same plane with H = H_f, W = W_f, frame_width = fw_f: SciPy's
 *   labelling, labels in raster order of the first pixel, the same statistics and table rows; a row over capacity keeps
 *   -1, runs, 0, 0, 0, 0, 0, 0, an all-zero output plane and zero table rows.
 * CHECKED ON THE DEVICE, per row, every value wave-uniform and before an address is formed from it, in this order: image_index[n]
 *   inside [0, P); the frame row against the la3d_frame contract and the bounds (the check of the fit); bits_offsets[n] >= 0 and a
 *   multiple of 4; out_offsets[n] likewise (with out_bits); then that the planes end inside their buffers: bits_offsets[n] + words
 *   <= bits_words and out_offsets[n] + words <= out_words.  A refused row reads no plane word, writes no plane word and gets the
 *   statistics row -2, 0, 0, 0, 0, 0, 0, 0 and zero table rows (both addressed by n alone): -2 tells it from a row over capacity
 *   (-1, runs, ...) and from an empty plane (0, 0, ...).  The other rows of the call are not affected by either.
 * workspace: la3d_components_workspace_bytes(B, H, max_runs) bytes with H the bound - the sizing call of la3d_components_bits serves
 *   both forms -, 4-byte aligned: one segment per row, sized by the bound.  Nothing depends on what it held before.  The dynamic LDS
 *   is 4 * max_runs bytes up to 32768 runs, as in the uniform form.  One kernel, one workgroup per row, no host synchronisation, no
 *   allocation, no atomics beyond integer min / max / add: the call can be captured into a HIP graph.
 * Refused before any launch, for B == 0 too, in this order - LA3D_ERR_ARG: a NULL block or a bad struct_size; B, P < 0, bounds H, W
 *   <= 0; connectivity not 4 or 8; largest not 0 or 1; min_area < 0; max_runs < 1; max_components < 0; components without
 *   max_components > 0; out_bits, stats and components all NULL; nonzero reserved; bits_words < 0, out_words < 0 with out_bits; bits or
 *   out_bits not 16-byte aligned; bits_offsets, out_offsets or frames not 8-byte aligned; stats, components, workspace or image_index
 *   not 4-byte aligned; the word ranges [bits, bits + bits_words) and [out_bits, out_bits + out_words) overlapping (the output is
 *   gathered from the runs of the input: the call cannot work in place); and with B > 0: bits, bits_offsets, image_index, workspace or
 *   - with P > 0 - frames NULL, out_offsets NULL with out_bits.  LA3D_ERR_UNSUPPORTED: bounds with H * roundup32(W) > 1048576;
 *   max_runs > 524288.  B == 0 then returns 0 with nothing launched.  P == 0 with B > 0: every row is refused on the device (-2 rows). */
typedef struct la3d_components_frames_args {
  int32_t struct_size;                                   /* sizeof(la3d_components_frames_args) of the caller */
  int32_t B, P;
  int32_t H, W;                                          /* bounds of the table */
  int32_t connectivity, min_area, largest, max_runs, max_components;   /* as in la3d_components_args */
  int32_t reserved[2];                                   /* 0 */
  const uint32_t* bits; int64_t bits_words; const int64_t* bits_offsets;      /* the buffer, its words, dev [B] */
  const la3d_frame* frames; const int32_t* image_index;                        /* dev [P], dev [B] */
  uint32_t* out_bits; int64_t out_words; const int64_t* out_offsets;          /* NULL: statistics only; dev [B] */
  int32_t* stats;                                        /* dev [B][8] or NULL */
  int32_t* components;                                   /* dev [B][max_components][5] or NULL */
  void* workspace; void* stream;
} la3d_components_frames_args;
int la3d_components_bits_frames(const la3d_components_frames_args* args);

/* ---- depth gate on bit planes ------------------------------------------------------------------------------------------
 * What the depth says about a mask: the depth + mask fit takes every set pixel and its extents are plain minima and maxima, so one
 * wrong depth under a mask sets the size of the box - a fill value of the depth stage (the reference's align_depth writes 10000.0
 * where it cannot predict), or the few background pixels of a mask that bleeds over an occlusion edge.  la3d_open_bits removes by
 * shape, la3d_components_bits by component; this entry removes by DEPTH, for a batch of planes in one launch.
 * RULE, per instance, with d the float32 depth plane of its image and m its plane (image columns < frame_width only) - NumPy:
 *     valid = m & isfinite(d) & (d >= float32(near)) & (d <= float32(far))
 *     v     = d[valid]                                        float32
 *     med   = np.median(v)                                    float32; an even count averages the two middle values in float32
 *     mad   = np.median(np.abs(v - med))                      float32, same rule
 *     thr   = np.maximum(float32(k) * mad, float32(min_band)) one float32 product
 *     keep  = valid & (np.abs(d - med) <= thr)                one float32 subtraction per pixel
 *   k (finite, >= 0; 4.5 is about three sigma of a Gaussian, and a surface whose depths are spread uniformly over their range keeps
 *   every pixel) scales the band; min_band (finite, >= 0) is a floor for the band in depth units - needed where quantised depth
 *   gives mad == 0, which with min_band = 0 keeps only the pixels AT the median; near / far (-inf / +inf: none; NaN refused) bound
 *   the depths that count at all - far = 9999 handles the reference's fill by itself.  No valid pixel: the output plane is empty and
 *   med, mad, thr are NaN.  Magnitudes whose float32 sum or difference overflows, and subnormal depths, are outside the contract.
 * INPUT.  B planes of "masks as bit planes" (H rows, pitch W, frame_width image columns), bits_plane_stride words apart; depth:
 *   float32 planes of pitch W (as wide as the planes are STORED), depth_plane_stride elements apart - 0: one plane shared by every
 *   instance -; instance b reads plane image_index[b], or plane b when image_index is NULL.  The index is not range-checked.
 * OUTPUT.  out_bits (NULL: statistics only, no plane is written): the plane of keep in the input's geometry, out_plane_stride words
 *   apart - all la3d_mask_bits_words(H, W) words of it are written; every bit of a column >= frame_width, and beyond H * W in the
 *   last word, is written as zero whatever the input held there.  counts[b] (i32 [3]) = area_in (the set bits of the image columns),
 *   n_valid, area_out.  levels[b] (f32 [3]) = med, mad, thr.  Planes and counts equal the rule exactly, levels value for value (the
 *   sign of a zero aside).
 * IN PLACE.  out_bits may be EXACTLY the input (out_bits == mask_bits with equal strides): a workgroup holds its plane in LDS before
 *   it stores a word.  Word ranges [mask_bits, mask_bits + B * bits_plane_stride) and [out_bits, out_bits + B * out_plane_stride)
 *   that overlap in any other way are refused.
 * One kernel, one 512-thread workgroup per instance: the plane is copied into LDS once, both medians are exact selections on
 *   order-preserving keys (the second over |d - med| re-derived from memory), the last pass writes the words.  Integer LDS atomics
 *   only, no workspace, no allocation, no host synchronisation: the call can be captured into a HIP graph, and a plane's result
 *   depends neither on the rest of the batch nor on the run.
 * Refused before any launch, in this order - LA3D_ERR_ARG: a NULL block or a bad struct_size; B < 0, H, W <= 0; frame_width outside
 *   [0, W]; k or min_band negative or not finite; near or far NaN; nonzero reserved; a stride that is negative or - unless 0 - shorter
 *   than a plane (0: depth - one shared plane; bits, out - the words of a plane).  LA3D_ERR_UNSUPPORTED: a frame whose bit image,
 *   chunk list and selection buffers exceed one CU's 160 KiB of LDS - every H * W up to 857728 stored pixels fits (640 x 1280 =
 *   819200 does).  B == 0 then returns 0 with no launch.  With B > 0, LA3D_ERR_ARG: out_bits, counts and levels all NULL; depth or
 *   mask_bits NULL; a pointer that is not 4-byte aligned; planes that overlap without being the same planes. */
typedef struct la3d_depth_gate_args {                    /* 120 bytes */
  int32_t struct_size;                                   /* sizeof(la3d_depth_gate_args) of the caller */
  int32_t B, H, W;                                       /* W: the pitch of the planes as stored, bits and depth alike */
  int32_t frame_width;                                   /* 0 = W */
  float k, min_band, near, far;
  int32_t reserved;                                      /* 0 */
  const float* depth; int64_t depth_plane_stride;        /* dev f32, pitch W; elements between planes, 0 = one shared plane */
  const int32_t* image_index;                            /* dev [B] or NULL */
  const uint32_t* mask_bits; int64_t bits_plane_stride;  /* bit planes; words between planes, 0 = the words of a plane */
  uint32_t* out_bits; int64_t out_plane_stride;          /* NULL: statistics only; words between planes, 0 = the words of a plane */
  int32_t* counts;                                       /* dev [B][3] or NULL */
  float* levels;                                         /* dev [B][3] or NULL */
  void* stream;
} la3d_depth_gate_args;
int la3d_depth_gate_bits(const la3d_depth_gate_args* args);

/* la3d_depth_gate_bits_frames: the gate for the planes of images of DIFFERENT sizes, over depth as it is stored - float32, float16 or
 * uint16 -, in one call ("images of different sizes in one call": the la3d_frame table, P rows, and its bounds H, W - the largest rows
 * and the largest pitch).  One k, min_band, near and far per call.
 * INPUT.  Row n belongs to image image_index[n]; its plane lies at bits + bits_offsets[n] and holds the H_f * W_f / 32 words of that
 *   image's frame row (H_f rows, pitch W_f - a multiple of 32 -, frame_width fw_f image columns).  Columns at and beyond fw_f count as
 *   zero whatever the plane holds.  bits_words: the words of the buffer at bits.  The depth plane of the image lies depth_offset
 *   elements into the depth buffer, pitch W_f, H_f rows: exactly one of `depth` (float32, 16-byte aligned) and `depth16` is given.
 *   With depth16 the rules of la3d_fit_instances_frames_depth16 apply: plane_stride 0, an 8-byte aligned base, depth_offset counted
 *   in 16-bit ELEMENTS; the float32 value of a stored word is the one of "16-bit depth planes" - F16 exact, U16 ONE rounded
 *   float32(x) * scale that is never contracted into the subtraction of the median, a stored 0 a NaN (hence not valid) with
 *   LA3D_DEPTH_ZERO_IS_HOLE - and from that value on the RULE above applies unchanged: a 16-bit call gives, word for word, what the
 *   float32 call gives on the up-converted planes.  depth_elems: the elements of the depth buffer.
 * OUTPUT.  out_bits (NULL: statistics only): the plane of row n at out_bits + out_offsets[n], in the input's geometry.  A conforming
 *   row writes exactly the H_f * W_f / 32 words of its plane - the bits of the padding columns zero - and nothing else; out_words: the
 *   words of the buffer at out_bits.  counts[n] (i32 [3]) and levels[n] (f32 [3]) as in la3d_depth_gate_bits.
 * CONFORMING ROWS get what la3d_depth_gate_bits gives for the same plane with H = H_f, W = W_f, frame_width = fw_f over the same depth.
 * IN PLACE.  The output may be EXACTLY the input - out_bits == bits, out_words == bits_words and out_offsets the very pointer given
 *   as bits_offsets: a workgroup holds its plane in LDS before it stores a word.  Word ranges [bits, bits + bits_words) and [out_bits,
 *   out_bits + out_words) that overlap in any other way are refused.  The planes of different rows must not overlap each other: the
 *   caller's contract, as for la3d_components_bits_frames.
 * CHECKED ON THE DEVICE, per row, every value wave-uniform and before an address is formed from it, in this order: image_index[n]
 *   inside [0, P); the frame row against the la3d_frame contract and the bounds (the check of the fit); bits_offsets[n] >= 0 and a
 *   multiple of 4; bits_offsets[n] + words <= bits_words; with out_bits, out_offsets[n] by the same two rules against out_words; then
 *   depth_offset + H_f * W_f <= depth_elems.  A refused row reads no plane word and no depth, writes no plane word and gets counts
 *   -2, 0, 0 and levels NaN, NaN, NaN (both addressed by n alone): -2 is the marker of la3d_open_bits_frames and
 *   la3d_components_bits_frames; an empty plane has 0, 0, 0.  The other rows of the call are not affected.
 * One kernel - la3d_depth_gate_bits' own, per row geometry -, one 512-thread workgroup per row; its dynamic LDS is sized by the
 *   BOUNDS (bit image, chunk list and selection buffers of H * roundup32(W) stored pixels: 94 KB at 640 x 640, one workgroup per CU
 *   from 80 KB on).  Integer LDS atomics only, no workspace, no allocation, no host synchronisation: the call can be captured into a
 *   HIP graph.
 * Refused before any launch, for B == 0 too, in this order - LA3D_ERR_ARG: a NULL block or a bad struct_size; B, P < 0, bounds H, W
 *   <= 0; k or min_band negative or not finite; near or far NaN; nonzero reserved; both or neither of depth and depth16; a bad
 *   la3d_depth16 block (struct_size, dtype, scale, flags, nonzero plane_stride, NULL planes); depth_elems < 0, bits_words < 0, out_words < 0
 *   with out_bits; bits or out_bits not 16-byte aligned; float32 depth not 16-byte, 16-bit planes not 8-byte aligned; bits_offsets,
 *   out_offsets or frames not 8-byte aligned; image_index, counts or levels not 4-byte aligned; out_bits, counts and levels all NULL;
 *   buffers that overlap without being the same planes; and with B > 0: bits, bits_offsets, image_index or - with P > 0 - frames
 *   NULL, out_offsets NULL with out_bits.  LA3D_ERR_UNSUPPORTED: bounds with H * roundup32(W) > 857728 stored pixels (the LDS of
 *   la3d_depth_gate_bits).  B == 0 then returns 0 with nothing launched.  P == 0 with B > 0: every row is refused on the device. */
typedef struct la3d_depth_gate_frames_args {             /* 152 bytes */
  int32_t struct_size;                                   /* sizeof(la3d_depth_gate_frames_args) of the caller */
  int32_t B, P;
  int32_t H, W;                                          /* bounds of the table */
  float k, min_band, near, far;                          /* as in la3d_depth_gate_args */
  int32_t reserved;                                      /* 0 */
  const float* depth;                                    /* dev f32 buffer, 16-byte aligned, or NULL */
  const la3d_depth16* depth16;                           /* 16-bit buffer (plane_stride 0, 8-byte aligned), or NULL: exactly one of the two */
  int64_t depth_elems;                                   /* elements of the depth buffer */
  const la3d_frame* frames; const int32_t* image_index;                        /* dev [P], dev [B] */
  const uint32_t* bits; int64_t bits_words; const int64_t* bits_offsets;      /* the buffer, its words, dev [B] */
  uint32_t* out_bits; int64_t out_words; const int64_t* out_offsets;          /* NULL: statistics only; dev [B] */
  int32_t* counts;                                       /* dev [B][3] or NULL */
  float* levels;                                         /* dev [B][3] or NULL */
  void* stream;
} la3d_depth_gate_frames_args;
int la3d_depth_gate_bits_frames(const la3d_depth_gate_frames_args* args);

/* ---- mask overlap on bit planes ----------------------------------------------------------------------------------------
 * What relates two planes of one image: for every GROUP g (an image) and every pair of a row i of A_g and a row j of B_g
 *     inter[offsets[g] + i * nb_g + j] = popcount(A_i & B_j)   over the words [0, nwords) of the planes,
 * with the planes' own areas popcount(A_i), popcount(B_j) from the same loads, and on request
 *     iou = (double)inter / (double)den,  den = area_a + area_b - inter (LA3D_OVERLAP_IOU) | min(area_a, area_b) (LA3D_OVERLAP_IOM) |
 *           area_a (LA3D_OVERLAP_IOA);  den == 0 gives 0.0.
 * The planes are those of "masks as bit planes", whatever packer made them.  FRAME CONTRACT: the padding bits of a plane are zero
 * (every packer writes them so) - ALL words [0, nwords) are counted.  The rows of a group are contiguous in A and in B; B == NULL is
 * the SELF form (B is A): only the tiles on and above the diagonal are computed and mirrored, the full square matrix is written.
 *
 * la3d_mask_overlap_plan - HOST, no device.  From the rows per group of A and of B (counts_b NULL: self) and the words per group
 *   (group_words NULL: nwords for every group) it writes offsets[G + 1] (offsets[g + 1] - offsets[g] = na_g * nb_g, row-major (i, j))
 *   and the TILE TABLE: one la3d_overlap_tile per workgroup - up to 8 x 8 planes of one group and the words [w0, w1) of them.  Every
 *   (group, i, j, word) of the call lies in exactly one tile (self form: every i <= j, the mirror tile standing for the rest).  A call
 *   with few tiles gets the word range of each tile split into chunks (whole multiples of 1024 words), so that one image still fills
 *   the chip; the chunks of a tile follow each other in the table.  A group whose other side is empty keeps tiles with nj (ni) = 0:
 *   they carry its areas.  The caller uploads the rows it got (8-byte aligned) and hands them to la3d_mask_overlap unchanged - the
 *   kernels trust the table.  tiles NULL: count only.  Returns the number of tiles; -1 (LA3D_ERR_ARG) when capacity is smaller or an
 *   argument is bad (G < 0, a negative count or word count, offsets NULL); LA3D_ERR_UNSUPPORTED beyond the limits below.
 * la3d_mask_overlap_workspace_bytes(ntiles) - HOST: 320 bytes per tile (its 64 pair counts and 16 areas); 0 for ntiles <= 0.
 * la3d_mask_overlap - two kernels on the caller's stream: one workgroup per tile leaves its partial counts in the workspace, then
 *   one per tile sums the chunks and writes inter, area_a, area_b (i32) and - iou != NULL - iou (f64).  No atomics, nothing is
 *   pre-cleared by the caller, every element of [0, offsets[G]) is written exactly once and nothing else is; no host synchronisation:
 *   with its table and workspace the call can be captured into a HIP graph.  Planes are addressed in one of two ways:
 *   UNIFORM (frames NULL): plane of row r at a_bits + r * a_stride, nwords words, 4-byte aligned; a 16-byte aligned base with a
 *     stride that is a multiple of 4 (both sides) is read in 16-byte groups, anything else word by word - never a misaligned vector
 *     load -, with the same results.
 *   FRAMES (frames != NULL): plane of row r at a_bits + a_offsets[r] (dev i64), group g IS image g of the table (G == P) and its
 *     planes hold the H_g * W_g / 32 words of frames[g]; a_bits / b_bits 16-byte aligned.  CHECKED ON THE DEVICE, per row, before an
 *     address is formed: the frame row of its group (the check of the fit, against the bounds H, W) and that its words are the
 *     plan's; a_image_index[r] == g; a_offsets[r] >= 0 and a multiple of 4; a_offsets[r] + words <= a_words.  A refused row reads
 *     nothing; every pair of it gets inter -1 and iou NaN, its area is -1.  Never through the call status.
 *   LA3D_ERR_ARG before any launch: a bad struct_size or kind, G or a row count < 0, NULL or misaligned pointers with work to do,
 *     a stride below nwords, frames with G != P or bounds <= 0.  LA3D_ERR_UNSUPPORTED: nwords (frames: H * W / 32 of the bounds) above
 *     2^23 - H * W_stored <= 2^28, so a count fits int32 -, npairs above 2^31 - 1.  ntiles == 0: success, nothing is launched.
 * la3d_mask_nms - greedy mask NMS on a SELF overlap, one workgroup per group: the rows of group g are visited in the order
 *   order[row_offsets[g] .. row_offsets[g + 1]) (global row indices; an entry outside its group's rows is skipped).  A kept row t
 *   suppresses a later row u iff labels is NULL or labels[t] == labels[u], den(t, u) > 0 and
 *       (double)inter[t, u] > thr * (double)den(t, u)            - a multiply, never a division: host and device agree bit for bit -
 *   den by kind (LA3D_OVERLAP_IOU or LA3D_OVERLAP_IOM).  keep (u8 [B]) is written for every row: 1 kept, 0 otherwise.  A row with
 *   area -1 is never kept and suppresses nothing; so is a row the order does not name.  At most 46340 rows per group (its matrix
 *   has at most 2^31 - 1 pairs); no synchronisation, capturable. */
#define LA3D_OVERLAP_NONE 0
#define LA3D_OVERLAP_IOU 1
#define LA3D_OVERLAP_IOM 2
#define LA3D_OVERLAP_IOA 3
#define LA3D_OVERLAP_MIRROR 1   /* la3d_overlap_tile::flags - self form, above the diagonal: the tile is also written transposed */
#define LA3D_OVERLAP_AREA_A 2   /*   the tile writes area_a of its rows of A */
#define LA3D_OVERLAP_AREA_B 4   /*   the tile writes area_b of its rows of B */
typedef struct la3d_overlap_tile {   /* 64 bytes */
  int32_t g;                         /* group */
  int32_t i0, j0;                    /* first row of A / of B, within the group */
  int32_t ni, nj;                    /* rows of A / of B: 0 .. 8 */
  int32_t row_a, row_b;              /* the same first rows, counted over the whole call */
  int32_t w0, w1;                    /* words [w0, w1) of the planes */
  int32_t nw;                        /* words of a plane of the group */
  int32_t chunk, nchunks;            /* this tile is chunk `chunk` of `nchunks` consecutive rows of the table */
  int32_t nb;                        /* nb_g: the row length of the group's matrix */
  int32_t flags;                     /* LA3D_OVERLAP_MIRROR | LA3D_OVERLAP_AREA_A | LA3D_OVERLAP_AREA_B */
  int64_t out0;                      /* offsets[g] */
} la3d_overlap_tile;
typedef struct la3d_mask_overlap_args {
  int32_t struct_size;                                   /* sizeof(la3d_mask_overlap_args) of the caller */
  int32_t G;                                             /* groups */
  int32_t kind;                                          /* LA3D_OVERLAP_*: the denominator of iou (read with iou != NULL) */
  int32_t P, H, W;                                       /* frames form: rows of the table, its bounds */
  int64_t rows_a, rows_b;                                /* rows of A, of B (self form: rows_b is not read) */
  const uint32_t* a_bits; const uint32_t* b_bits;        /* b_bits NULL: the self form - every b_* field is then A's */
  int64_t a_stride, b_stride; int64_t nwords;            /* uniform form */
  const la3d_frame* frames;                              /* dev [P] | NULL: the frames form */
  const int64_t* a_offsets; const int64_t* b_offsets;    /* dev [rows], frames form */
  const int32_t* a_image_index; const int32_t* b_image_index;   /* dev [rows], frames form */
  int64_t a_words, b_words;                              /* words of the buffers at a_bits / b_bits, frames form */
  const la3d_overlap_tile* tiles; int64_t ntiles;        /* dev: the table of la3d_mask_overlap_plan */
  int64_t npairs;                                        /* offsets[G] of the plan */
  int32_t* inter;                                        /* dev [npairs] */
  int32_t* area_a; int32_t* area_b;                      /* dev [rows_a], [rows_b]; self form: area_b may be NULL or area_a */
  double* iou;                                           /* dev [npairs] | NULL */
  void* workspace; void* stream;
} la3d_mask_overlap_args;
typedef struct la3d_mask_nms_args {
  int32_t struct_size;                                   /* sizeof(la3d_mask_nms_args) of the caller */
  int32_t G;                                             /* groups */
  int32_t kind;                                          /* LA3D_OVERLAP_IOU | LA3D_OVERLAP_IOM */
  int32_t reserved;
  int64_t B;                                             /* rows */
  const int32_t* inter; const int32_t* area;             /* dev: a self overlap and its areas */
  const int64_t* offsets;                                /* dev [G + 1]: the plan's offsets */
  const int32_t* row_offsets;                            /* dev [G + 1]: the first row of each group, row_offsets[G] = B */
  const int32_t* order;                                  /* dev [B] */
  const int32_t* labels;                                 /* dev [B] | NULL */
  double thr;
  uint8_t* keep;                                         /* dev [B] */
  void* stream;
} la3d_mask_nms_args;
int64_t la3d_mask_overlap_plan(int32_t G, const int32_t* counts_a, const int32_t* counts_b /* NULL: self */,
                               const int64_t* group_words /* NULL: nwords for all */, int64_t nwords,
                               la3d_overlap_tile* tiles /* host [capacity] | NULL: count only */, int64_t capacity,
                               int64_t* offsets /* host [G + 1] */);
size_t la3d_mask_overlap_workspace_bytes(int64_t ntiles);
int la3d_mask_overlap(const la3d_mask_overlap_args* args);
int la3d_mask_nms(const la3d_mask_nms_args* args);

/* ---- assignment on the device (reference stage 8: hungarian_matching, src/tools/combine_results.py:126-144) ----------------
 * la3d_assign - for every GROUP g (an image) the rectangular linear sum assignment of the na_g x nb_g matrix at cost + offsets[g],
 *   row-major (row i of A, row j of B): the layout of la3d_mask_overlap's inter / iou and of la3d_iou_matrix_groups.  na_g, nb_g are
 *   the differences of row_offsets_a / row_offsets_b (as in la3d_mask_nms).  cost_dtype LA3D_ASSIGN_F64, or LA3D_ASSIGN_I32 (the
 *   `inter` of a mask overlap; converted to double, which is exact).  maximize 1: the matrix is negated first.
 *   The arithmetic is SciPy's (scipy.optimize.linear_sum_assignment, 1.15: shortest augmenting paths on float64, additions and
 *   subtractions only), step for step, TIES INCLUDED - most pairs of an image score 0, so ties decide real matrices: na > nb solves
 *   the transpose; rows in ascending order; of the remaining columns with the least path cost an unassigned one at the highest
 *   position of SciPy's `remaining` list wins, else the one at the lowest position.  The result is SciPy's (rows, cols) exactly.
 *   One wave per group, no barriers, no atomics, no workspace, no allocation, no host synchronisation: the call can be captured.
 *   Column j lives in lane j % 64 (path cost, dual, row, predecessor, position: registers), the duals of the rows in LDS; a group
 *   of at most LA3D_ASSIGN_STAGE_MAX elements is staged into LDS in the solver's orientation, a larger one is read where it lies -
 *   the same results either way.
 *   col_of_row i32 [rows_a]: the column within its group, -1 if none; row_of_col i32 [rows_b] likewise; status i32 [G]:
 *     0 LA3D_ASSIGN_OK          assigned (an empty side: all -1)
 *     1 LA3D_ASSIGN_INVALID     an entry is NaN, or -inf after the sign of maximize  (SciPy: "matrix contains invalid numeric
 *                               entries"; +inf is legal)
 *     2 LA3D_ASSIGN_INFEASIBLE  (SciPy: "cost matrix is infeasible")
 *     3 LA3D_ASSIGN_TOO_LARGE   max(na, nb) > LA3D_ASSIGN_MAX_N
 *     4 LA3D_ASSIGN_BROKEN      the tables are broken: a negative count, a row range outside [0, rows_a] / [0, rows_b], or a matrix
 *                               outside [0, ncost) - checked wave-uniformly before any address is formed from these values; such a
 *                               group gets ONLY its status written
 *   With status 1 - 3 every row and column of the group gets -1.  Every output element of a well-formed group is written exactly once.
 *   LA3D_ERR_ARG before any launch, in this order: a NULL block or a bad struct_size; G, rows_a, rows_b or ncost < 0; a bad
 *   cost_dtype, or maximize not 0 or 1; (G == 0: success, nothing launched;) NULL offsets, row_offsets_a, row_offsets_b, status, or
 *   cost / col_of_row / row_of_col with ncost / rows_a / rows_b > 0; cost (8 bytes for F64, 4 for I32), offsets (8) or the i32
 *   pointers (4) misaligned.
 * la3d_iou_matrix_groups - la3d_iou_matrix for G groups in one launch: out[offsets[g] + i * nb_g + j] = iou2D(A row
 *   row_offsets_a[g] + i, B row row_offsets_b[g] + j), the same device expression: every group's values are bit-identical to a
 *   la3d_iou_matrix call on it.  One thread per element of [0, npairs) finds its group in offsets (npairs = offsets[G], known to the
 *   host); an element whose tables are broken (it lies in no group's matrix, or its rows outside [0, rows_a) / [0, rows_b)) gets NaN
 *   and reads no box.  LA3D_ERR_ARG: NULL block, bad struct_size, G / rows / npairs < 0, NULL or misaligned pointers with npairs > 0. */
#define LA3D_ASSIGN_F64 0
#define LA3D_ASSIGN_I32 1
#define LA3D_ASSIGN_MAX_N 256        /* rows and columns of a group: four columns per lane */
#define LA3D_ASSIGN_STAGE_MAX 2048   /* elements of a group's matrix that are staged in LDS (16 KiB of doubles: eight waves per CU) */
#define LA3D_ASSIGN_OK 0
#define LA3D_ASSIGN_INVALID 1
#define LA3D_ASSIGN_INFEASIBLE 2
#define LA3D_ASSIGN_TOO_LARGE 3
#define LA3D_ASSIGN_BROKEN 4
typedef struct la3d_assign_args {
  int32_t struct_size;                                   /* sizeof(la3d_assign_args) of the caller */
  int32_t G;                                             /* groups */
  const void* cost;                                      /* dev: the flat cost buffer */
  int32_t cost_dtype;                                    /* LA3D_ASSIGN_F64 | LA3D_ASSIGN_I32 */
  int32_t reserved0;
  int64_t ncost;                                         /* elements of cost */
  const int64_t* offsets;                                /* dev [G + 1] */
  const int32_t* row_offsets_a; const int32_t* row_offsets_b;   /* dev [G + 1] */
  int64_t rows_a, rows_b;                                /* total rows of A, of B */
  int32_t maximize;                                      /* 0 | 1 */
  int32_t reserved1;
  int32_t* col_of_row;                                   /* dev [rows_a] */
  int32_t* row_of_col;                                   /* dev [rows_b] */
  int32_t* status;                                       /* dev [G] */
  void* stream;
} la3d_assign_args;
typedef struct la3d_iou_groups_args {
  int32_t struct_size;                                   /* sizeof(la3d_iou_groups_args) of the caller */
  int32_t G;                                             /* groups */
  const double* boxes_a; const double* boxes_b;          /* dev f64 [rows_a][4], [rows_b][4], xyxy */
  int64_t rows_a, rows_b;
  const int32_t* row_offsets_a; const int32_t* row_offsets_b;   /* dev [G + 1] */
  const int64_t* offsets;                                /* dev [G + 1] */
  int64_t npairs;                                        /* offsets[G] */
  double* out;                                           /* dev f64 [npairs] */
  void* stream;
} la3d_iou_groups_args;
int la3d_assign(const la3d_assign_args* args);
int la3d_iou_matrix_groups(const la3d_iou_groups_args* args);

/* HOST helper: COCO compressed RLE string (pycocotools rleFrString) -> run lengths.  Returns the number of
 * counts written, or -1 (malformed string / cap too small). */
int la3d_rle_from_string_host(const char* s, int64_t len, int32_t* counts, int cap);
/* HOST helper, the inverse: run lengths -> COCO compressed RLE string (pycocotools rleToString), byte for byte, without a
 * terminating NUL.  Returns the bytes written (at most 7 per count), or -1 (bad argument / cap too small: out then holds a prefix). */
int64_t la3d_rle_to_string_host(const int32_t* counts, int64_t n, char* out, int64_t cap);

/* ---- box consumers: the step immediately downstream of the path ----------------------------
 * Reference src/tools/combine_results.py: the 8 corners of each record are projected with the image's K
 * (project_to_2d, :105-108), bbox2D_proj = [min_x, min_y, max_x, max_y] and bbox2D_trunc = its clamp to
 * [0,width] x [0,height] (:238-252).  records dev f64 [B][39] (as written by the fit calls), K dev f64 (9 per
 * image, k_stride 0 = shared), image_index dev i32 [B] | NULL; out dev f64 [B][8] = proj(4), trunc(4); a box with a
 * NaN projection gives 8 NaNs. */
int la3d_project_boxes(const double* records, const double* K, int32_t k_stride, const int32_t* image_index, int B,
                       double width, double height, double* out, void* stream);

/* iou2D (:111-124) of every pair of xyxy boxes: a dev f64 [na][4], b dev f64 [nb][4] -> out dev f64 [na][nb]
 * (negated = the Hungarian cost matrix of :131-135). */
int la3d_iou_matrix(const double* boxes_a, int na, const double* boxes_b, int nb, double* out, void* stream);

/* ---- masked depth statistics ------------------------------------------------------------------
 * Reference src/util.py:476-486 (align_to_depth_match): overlap = mask & render_mask;
 * scale = np.median(depth_map[overlap] / depth_render[overlap])  (float32 arithmetic, float32 result).
 * num   dev f32 planes (plane of instance n = image_index[n] or n; stride in floats, 0 = one shared plane)
 * den   dev f32 [B][H*W];  mask_a dev u8 [B][H*W];  mask_b dev u8 [B][H*W] | NULL (non-zero = True)
 * median dev f32 [B] (NaN when the overlap is empty or a ratio is NaN, as np.median);  count dev i32 [B].
 * H*W <= 819200 (the overlap bit image, the chunk list and the key buffer share one CU's LDS); larger frames: LA3D_ERR_UNSUPPORTED. */
int la3d_masked_ratio_median(const float* num, int64_t num_plane_stride, const int32_t* image_index, const float* den,
                             const uint8_t* mask_a, const uint8_t* mask_b, int B, int H, int W, float* median,
                             int32_t* count, void* stream);

/* align_depth (reference src/batch_scripts/depth.py:52-92), the data-parallel parts around its scikit-learn RANSAC fit:
 * la3d_align_select compacts, in row-major order, the pixels with ~isinf(relative) & (metric < max_valid_depth) [& mask]
 * into relative_out / metric_out (dev f32, capacity n) — what the reference feeds regressor.fit (:69-78) — and writes
 * their number to count (dev i64).  workspace: dev scratch of la3d_align_workspace_bytes(n) bytes.
 * la3d_align_apply writes depth = full(fill); depth[sel] = relative[sel] * coef + intercept in float32 with
 * sel = mask when given, else ~isinf(relative) (:82-90; fill is 10000.0 there). */
size_t la3d_align_workspace_bytes(int64_t n);
int la3d_align_select(const float* relative, const float* metric, const uint8_t* mask, int64_t n, float max_valid_depth,
                      float* relative_out, float* metric_out, int64_t* count, void* workspace, void* stream);
int la3d_align_apply(const float* relative, const uint8_t* mask, int64_t n, float coef, float intercept, float fill,
                     float* out, void* stream);
/* la3d_align_select for P frames of n pixels each in ONE call (three launches for the whole batch instead of three per frame plus an
 * 8-byte read-back each; the reference loops over images, src/batch_scripts/depth.py:138-160): relative / metric dev f32 [P][n],
 * mask dev u8 [P][n] | NULL; relative_out / metric_out dev f32 [P][n] (frame p's selection at [p][0 .. counts[p]), row-major order
 * kept); counts dev i64 [P] - left on the device; workspace: P * la3d_align_workspace_bytes(n) bytes.  P <= 65535. */
int la3d_align_select_batch(const float* relative, const float* metric, const uint8_t* mask, int P, int64_t n,
                            float max_valid_depth, float* relative_out, float* metric_out, int64_t* counts, void* workspace,
                            void* stream);

/* ---- depth alignment: RANSAC scale fit ---------------------------------------------------------------------------
 * The estimator between la3d_align_select_batch and the prediction scatter, for P frames in ONE call and without any host
 * synchronisation: scikit-learn's RANSACRegressor(LinearRegression(fit_intercept=False), min_samples=...) as align_depth calls it
 * (reference src/batch_scripts/depth.py:66-78) - the model y = a x with a median-based threshold.  Per frame, on the compacted float32
 * samples x = relative_sel[p][0 .. counts[p]), y = metric_sel[p][...]:
 *   m     = ceil(min_samples * n) in float64 for 0 < min_samples < 1, min_samples for an integer >= 1; m < 1 or m > n fails the fit
 *   thr   = median(|y - median(y)|), both medians as np.median of float32 data (an even count averages the middle values in float32)
 *   trial t with its subset of m sample indices: a_t = float32(sum xy / sum xx), sums in float64 (sum xx == 0: a_t = 0);
 *           pred = float32(x * a_t) for every sample (one rounded product), inliers |y - pred| <= thr in float32, k_t their number,
 *           score_t = R^2 over the inliers in float64 (fewer than two inliers: NaN; zero total variance: 1 if the residuals are 0, else 0)
 *   rule    scikit-learn's loop: k_best = 1, score_best = -inf; trial t is skipped if k_t < k_best or (k_t == k_best and score_t <
 *           score_best; a NaN compares false); otherwise it becomes the best and max_trials = min(max_trials, dynamic) with
 *           scikit-learn's _dynamic_max_trials(k_best, n, m, stop_probability) in float64; n_trials = trials looked at
 *   coef  = float32(sum xy / sum xx) over the inliers of the best trial, sums in float64
 *   status  0 fitted; 1 no sample (counts[p] == 0); 2 the fit failed - a non-finite sample, m outside [1, n] (or beyond m_cap), a subset
 *           index outside [0, n), counts[p] outside [0, n], no accepted trial: where the reference returns the metric depth.  coef is
 *           NaN, n_inliers 0 and best_trial -1 for a status other than 0.
 * Where this parts from scikit-learn.  (1) A ZERO THRESHOLD - one sample, constant y, more than half of the y equal: the inlier test is
 *   then the exact float32 equality y == float32(x * a_t) and hangs on the last bit of the slope, where float32(sum xy / sum xx) and
 *   LAPACK's float32 gelsd solution differ.  The library may fit such a frame (status 0, as few as one inlier) for which scikit-learn
 *   raises "no consensus set" and the reference returns the metric depth, or both fit with different coefficients (up to 1.7 x apart
 *   on constant y).  A caller who wants the reference's answer there treats thr == 0 as a failed fit.  (2) Magnitudes outside
 *   float32's range for sum y^2 (|y| of the order 1e19): scikit-learn scores float32 targets in float32, its scores overflow and
 *   its choice among trials of equal k is no longer by R^2; the scores here are float64.  (3) The residual squared in the score is
 *   the float32 residual of the inlier test or the float64 difference y - pred: left open, the two differ by 2^-24 relative at most
 *   (the kernels square the float32 one).  Everywhere else n_trials, the inlier set and coef (to 1.5e-6 relative) are scikit-learn's
 *   on the same subsets (tests/test_align_ransac_restatement.py); the kernels are held to the NumPy restatement in every class
 *   (oracle/campaigns/align_ransac.py).
 * Subsets: `subsets` dev i32 [P][max_trials][m_cap] - frame p, trial t uses the first m of its row (for a seeded scikit-learn draw made
 * on the host) -, or NULL: the kernels draw them from `seed`, counter-based and keyed by (seed, frame, trial): m DISTINCT indices per
 * trial (a keyed bijection of [0, n)).  The device draw is NOT NumPy's stream; la3d_align_ransac_subsets writes the subsets a seed
 * gives (rows padded with -1 behind m), and a fit fed those equals the seeded fit bit for bit.
 * A call is six launches on `stream`, allocates nothing and reads nothing back; every sum is merged in a fixed order, so a call is
 * reproducible run to run and a frame's result does not depend on the other frames of the batch.
 * workspace: la3d_align_ransac_workspace_bytes(P, n, max_trials) bytes, 16-byte aligned.
 * LA3D_ERR_ARG before any launch: a bad struct_size, negative P or n, max_trials < 1, min_samples <= 0 or a non-integer >= 1,
 *   stop_probability outside [0, 1], subsets with m_cap < 1, NULL or misaligned pointers with work to do.  LA3D_ERR_UNSUPPORTED:
 *   n > LA3D_ALIGN_RANSAC_MAX_N, max_trials > LA3D_ALIGN_RANSAC_MAX_TRIALS, P > 65535.
 * la3d_align_apply_batch: out[p] = full(fill); out[p][sel] = float32(relative[p] * coef[p]) with sel = mask when given, else
 * ~isinf(relative) - the expression of la3d_align_apply with a zero intercept, coef and status read from the device; a frame whose
 * status is not 0 gets metric[p] copied. */
#define LA3D_ALIGN_RANSAC_MAX_N (1 << 24)
#define LA3D_ALIGN_RANSAC_MAX_TRIALS 1024
typedef struct la3d_align_ransac_args {
  int32_t struct_size;        /* sizeof(la3d_align_ransac_args) of the caller */
  int32_t P;                  /* frames */
  int64_t n;                  /* samples a row holds (frames are n apart) */
  const float* relative_sel;  /* dev f32 [P][n] */
  const float* metric_sel;    /* dev f32 [P][n] */
  const int64_t* counts;      /* dev i64 [P] */
  double min_samples;
  double stop_probability;    /* 0.99 in scikit-learn */
  int32_t max_trials;         /* 100 in scikit-learn */
  int32_t m_cap;              /* columns of a subsets row */
  const int32_t* subsets;     /* dev i32 [P][max_trials][m_cap] | NULL: drawn on the device from seed */
  uint64_t seed;
  float* coef;                /* dev f32 [P] */
  int32_t* n_inliers;         /* dev i32 [P] */
  int32_t* n_trials;          /* dev i32 [P] */
  int32_t* best_trial;        /* dev i32 [P] */
  int32_t* status;            /* dev i32 [P] */
  void* workspace;
  void* stream;
} la3d_align_ransac_args;
size_t la3d_align_ransac_workspace_bytes(int P, int64_t n, int max_trials);
int la3d_align_ransac_batch(const la3d_align_ransac_args* args);
int la3d_align_ransac_subsets(const int64_t* counts, int P, double min_samples, int max_trials, uint64_t seed, int32_t* subsets,
                              int m_cap, void* stream);
int la3d_align_apply_batch(const float* relative, const float* metric, const uint8_t* mask, int P, int64_t n, const float* coef,
                           const int32_t* status, float fill, float* out, void* stream);

/* ---- ground plane: RANSAC plane fit ---------------------------------------------------------------------------------
 * The `ground` vector the fit entries take, from the depth itself: the dominant plane of P images of ONE size (float32 depth), found by
 * a batched RANSAC over back-projected grid samples.  Two entries, each a chain of launches on `stream` that allocates nothing and
 * reads nothing back, uses no floating-point atomics and merges every float sum in a fixed order: a frame's result does not depend on
 * the batch it is in, is the same from run to run, and a call with a given workspace can be captured in a graph.
 *
 * la3d_plane_select_batch - the samples.  Per image p the grid pixels (v, u) with v % step == 0, u % step == 0 (u < W, v < H), in
 *   raster order; a pixel is kept where isfinite(d) & d > 0 & near_depth <= d <= far_depth, compared on the float32 depth (0 and +inf
 *   keep every positive finite depth), and - with `candidates` - where its bit is set in plane p: P bit planes in the layout of
 *   "masks as bit planes" with a stored width cand_width that is a multiple of 32 and >= W, pixel (v, u) = bit v * cand_width + u of
 *   the plane, planes cand_plane_stride words apart (0: H * cand_width / 32); columns >= W are never read as image.  K: dev f64, one
 *   matrix (k_stride 0) or one per image (k_stride >= 9 doubles apart), inverted in the kernel as la3d_unproject_batch inverts it.
 *   With cap = ceil(H / step) * ceil(W / step):
 *     points  dev f64 [P][cap][3]   the rows of la3d_unproject_batch at the kept pixels, bit for bit
 *     pixel   dev i32 [P][cap]      v * W + u
 *     counts  dev i64 [P]
 *   Slots at and beyond counts[p] are not written.  workspace: la3d_plane_select_workspace_bytes(P, H, W, step) bytes, 4-byte aligned.
 *
 * la3d_plane_ransac_batch - the fit of P point sets: points dev f64 [P][n][3] and counts dev i64 [P], from the select or from any
 *   other source.  All arithmetic is float64 without contraction: the products and sums below are rounded one by one in the order
 *   written, and a trial's decisions use + - * only.
 *   Trial t of frame p uses the sample indices (i, j, k) = subsets[p][t][0..2] (dev i32 [P][max_trials][3]), or - subsets NULL - the
 *   device draw of the scale fit above with m = 3, keyed by (seed, p, t): la3d_align_ransac_subsets(counts, P, 3.0, max_trials, seed,
 *   out, 3, stream) writes exactly these rows, and a fit fed them equals the seeded fit bit for bit.  With a, b, c = points[i], [j], [k]:
 *     w = (b - a) x (c - a)      w_x = u_y v_z - u_z v_y, w_y = u_z v_x - u_x v_z, w_z = u_x v_y - u_y v_x  (u = b - a, v = c - a)
 *     s = w_x w_x + w_y w_y + w_z w_z
 *     skipped  when !(s > 0) or s is not finite (repeated indices, collinear triples, non-finite points), when an index lies outside
 *              [0, counts[p]), or when !(w_y w_y >= cos2_tilt * s): the prior against walls, cos2_tilt = cos^2 of the largest angle
 *              between the plane's normal and the camera's y axis (0: every orientation)
 *     sample q is an inlier iff its three coordinates are finite and e e <= (tol tol) s with
 *              e = w_x (x_q - a_x) + w_y (y_q - a_y) + w_z (z_q - a_z),  tol = thr_abs + thr_rel * z_q
 *     k_t = the number of inliers.  The best trial has the largest k_t, ties go to the lower t; all max_trials trials are judged.
 *   Refit over the inliers of the best trial: the mean mu from fixed-order sums, the covariance ABOUT mu in a second pass, n = the unit
 *     eigenvector of its smallest eigenvalue (cyclic Jacobi), negated if n_y > 0 - so that dot([0,-1,0], n) >= 0, the side the fit's
 *     flip rule keeps -, d = -(n . mu).  A non-finite refit reports the trial's plane: w / sqrt(s), oriented likewise, d = -(n . a).
 *   Reported under the REPORTED plane: r = n_x x + n_y y + n_z z + d, a final inlier iff its coordinates are finite and |r| <= tol;
 *     n_inliers = their number, rms = sqrt(mean r^2) over them, `inliers` (dev u8 [P][n] | NULL) their flags (every slot of a row is
 *     written).
 *     plane dev f64 [P][4] = (n_x, n_y, n_z, d);  k_trial, n_inliers, best_trial, status dev i32 [P];  rms dev f64 [P]
 *     status  0 fitted;  1 fewer than 3 samples;  2 no accepted trial, or k_trial < min_inliers (0 means the default, 3);
 *             3 a broken row (counts[p] outside [0, n]).  For a status other than 0 the plane is four NaN, best_trial -1, k_trial and
 *             n_inliers 0, rms NaN, and no flag is set.
 *   workspace: la3d_plane_ransac_workspace_bytes(P, n, max_trials) bytes, 16-byte aligned.
 *
 * LA3D_ERR_ARG before any launch: a bad struct_size; negative P, n, H or W; step < 1; max_trials < 1; thr_abs < 0, thr_rel < 0 or
 *   both zero (or not finite); cos2_tilt outside [0, 1]; min_inliers < 0; near_depth / far_depth NaN; k_stride neither 0 nor >= 9; a
 *   non-zero reserved; a cand_width that is no multiple of 32 or below W, a cand_plane_stride below the words of a plane; misaligned
 *   pointers; NULL pointers with work to do.  LA3D_ERR_UNSUPPORTED:
 *   max_trials > LA3D_PLANE_MAX_TRIALS, n > LA3D_PLANE_MAX_N, P > 65535, H * W > 2^30.  P == 0 is
 *   "nothing to do", ranked behind the argument checks. */
#define LA3D_PLANE_MAX_N (1 << 24)
#define LA3D_PLANE_MAX_TRIALS 1024
#define LA3D_PLANE_SEGMENT 1024         /* samples one workgroup of the candidates pass judges */
typedef struct la3d_plane_select_args {
  int32_t struct_size;        /* sizeof(la3d_plane_select_args) of the caller */
  int32_t P, H, W;            /* images, their size */
  int32_t step;               /* grid pitch in pixels, >= 1 */
  int32_t k_stride;           /* doubles between the K of consecutive images: 0 (shared) or >= 9 */
  float near_depth, far_depth;
  const float* depth;         /* dev f32 [P][H][W] */
  const double* K;            /* dev f64 [9] or [P][k_stride] */
  const uint32_t* candidates; /* dev bit planes | NULL */
  int64_t cand_plane_stride;  /* words; 0 = H * cand_width / 32 */
  int32_t cand_width;         /* stored width of a candidates row: a multiple of 32, >= W */
  int32_t reserved;           /* 0 */
  double* points;             /* dev f64 [P][cap][3] */
  int32_t* pixel;             /* dev i32 [P][cap] */
  int64_t* counts;            /* dev i64 [P] */
  void* workspace;
  void* stream;
} la3d_plane_select_args;
typedef struct la3d_plane_ransac_args {
  int32_t struct_size;        /* sizeof(la3d_plane_ransac_args) of the caller */
  int32_t P;                  /* point sets */
  int64_t n;                  /* samples a row holds (rows are n apart) */
  const double* points;       /* dev f64 [P][n][3] */
  const int64_t* counts;      /* dev i64 [P] */
  double thr_abs, thr_rel;    /* tol = thr_abs + thr_rel * z */
  double cos2_tilt;           /* [0, 1] */
  int32_t max_trials;
  int32_t min_inliers;        /* 0: 3 */
  const int32_t* subsets;     /* dev i32 [P][max_trials][3] | NULL: drawn on the device from seed */
  uint64_t seed;
  double* plane;              /* dev f64 [P][4] */
  int32_t* k_trial;           /* dev i32 [P] */
  int32_t* n_inliers;         /* dev i32 [P] */
  int32_t* best_trial;        /* dev i32 [P] */
  double* rms;                /* dev f64 [P] */
  int32_t* status;            /* dev i32 [P] */
  uint8_t* inliers;           /* dev u8 [P][n] | NULL */
  void* workspace;
  void* stream;
} la3d_plane_ransac_args;
size_t la3d_plane_select_workspace_bytes(int P, int H, int W, int step);
int la3d_plane_select_batch(const la3d_plane_select_args* args);
size_t la3d_plane_ransac_workspace_bytes(int P, int64_t n, int max_trials);
int la3d_plane_ransac_batch(const la3d_plane_ransac_args* args);

/* ---- sparse unprojection at match points -------------------------------------------------------
 * Reference src/matching/matcher.py:70-91: depth dev f32 [H][W] looked up at (int(v), int(u)) of each match
 * uv dev f64 [N][2]; matches whose depth is -1 (or that fall outside the frame) get valid = 0 and NaNs;
 * p = ((u'-cx) d/fx, (v'-cy) d/fy, d) with u' = flip-u, v' = flip-v when use_flip (the reference uses 512);
 * with R9 / T3 (HOST, both or neither): world = R (p - T)  (:88-89).  out dev f64 [N][3], valid dev i32 [N]. */
int la3d_unproject_matches(const float* depth, int H, int W, const double* uv, int N, double fx, double fy, double cx,
                           double cy, int use_flip, double flip, const double* R9, const double* T3, double* out,
                           int32_t* valid, void* stream);

/* Replaces estimate_bbox(in_pc, cat_name, ground_equ, method) for B point clouds at once —
 * reference src/util_3dbox.py:106-178 (caller :273-278, 500 mesh samples per object).
 * points   dev f64 [total][3];  offsets dev i64 [B+1] (cloud n = rows offsets[n]..offsets[n+1])
 * ground / sample_idx / out / status / aux as above (sample ranks index the cloud's rows).
 * method   LA3D_METHOD_PCA or LA3D_METHOD_CONVEX_HULL (_estimate_yaw_convex_hull, :189-224; at most 2048
 *          valid rows per cloud after sampling, else that box gets LA3D_BOX_UNSUPPORTED). */
int la3d_fit_points(const double* points, const int64_t* offsets, const double* ground,
                    const int32_t* sample_idx, int method, int B,
                    double* out, int32_t* status, double* aux, void* stream);

/* ---- instance point clouds ----------------------------------------------------------------------------------------------
 * The intermediate the fused fit never materialises: the per-instance cloud
 *     pts[n] = depth_to_points(depth[img(n)][None], K[img(n)])[mask[n]]          # src/util.py:52-75, :480-481
 * row-major (v ascending, then u ascending: NumPy's order), all B clouds packed into ONE array with an offsets array - exactly what
 * la3d_fit_points takes - for a PLY per object, another estimator, an aligner, or a look at what a box was fitted from.  Two stages
 * on the caller's stream; neither synchronises, so the chain can be captured into a HIP graph:
 *   la3d_instance_point_offsets(args)  counts[n] (i32 [B]) = the true pixels N_n of instance n - a non-zero byte of a u8 plane or a set
 *       bit of a bit plane, in columns < frame_width only -, offsets (i64 [B+1]) = the exclusive prefix of the rows each instance
 *       gets: N_n, or - with sample_idx - N_n if N_n <= 500, else 500 (the reference's rule, src/util_3dbox.py:123).  The scan runs on
 *       the device, deterministic, any B.  Per-band counts stay in `workspace` for the gather.  B == 0: offsets[0] = 0.
 *   la3d_gather_instance_points(args)  row offsets[n] + r of `points` = the point of the pixel of rank r of instance n (the rank of a
 *       pixel = the set pixels before it in row-major order, from popcount prefixes - never from atomics); with sample_idx and
 *       N_n > 500 row offsets[n] + j = the point of rank sample_idx[n][j] (repeated ranks repeat the row; a rank outside [0, N_n) gives a
 *       NaN row and pixel -1).  pixels (optional) = v * frame_width + u, the flat index in the unpadded image.
 * Both take the SAME block (the gather reads offsets and workspace as the first stage left them; points, pixels, status, capacity and
 * out_is_f64 are not read by the first stage, counts not by the second).
 * VALUE.  (d * Kinv) @ [u, v, 1] followed by the identity R, t multiply - the arithmetic of la3d_unproject_batch, K inverted in the
 *   kernel by the same elimination - so a row equals the row of la3d_unproject_batch's output bit for bit (float32 output: the cast of
 *   the float64 value).  NaN, inf, zero and negative depths are kept as they come (a NaN / inf depth poisons its row as there): this is
 *   the cloud BEFORE estimate_bbox drops anything.  16-bit planes: the value rules of "16-bit depth planes", unchanged - a call gives
 *   the rows of the float32 call on la3d_unpack_depth16's output, bit for bit.
 * FORMS.  frames == NULL: B instances of ONE H x W (W = pixels per row in memory; frame_width 0 = W, else the image columns).
 *   depth float32 planes depth_plane_stride floats apart (0 = one shared plane), or depth16 (its own plane_stride; depth_plane_stride 0);
 *   plane of instance n = image_index[n] or n, K likewise (k_stride 0 = shared).  mask: u8 planes mask_plane_stride bytes apart
 *   (0 = H*W; any width, any alignment - 16-byte groups where a band of rows is aligned, a general form behind it), or mask_bits: bit
 *   planes in the layout of la3d_pack_mask_bits, pitch W, bits_plane_stride words apart (0 = the words of a plane), 4-byte aligned.
 *   frames != NULL selects the FRAMES form (one pair of entries serves both): the ragged depth buffer + la3d_frame table (P rows) of
 *   la3d_fit_instances_frames / _frames_depth16 and bit planes at per-instance bits_offsets as in la3d_fit_instances_frames_bits;
 *   H, W are bounds, image_index is required, depth_plane_stride / frame_width / depth16->plane_stride must be 0, mask_bits 16-byte and
 *   the depth base 16-byte (16-bit: 8-byte) aligned.  An instance whose image index is outside [0, P), whose frame row breaks the
 *   la3d_frame contract or whose plane offset is negative or not a multiple of 4 gets count 0 in the first stage and
 *   LA3D_BOX_UNSUPPORTED (5) with nothing written in the second - decided on the device before any address is formed from the row.
 * STATUS (i32 [B], written by the gather).  The gather never writes outside rows [offsets[n], offsets[n+1]) of its own instance,
 *   whatever the masks hold: LA3D_CLOUD_NO_ROOM - the range does not lie within [0, capacity]: nothing of the instance is written;
 *   LA3D_CLOUD_MISMATCH - the mask count differs from the range length, or a band's count from what the first stage left in the
 *   workspace (the masks changed between the two calls): the range is filled only as far as it reaches.
 * workspace: la3d_instance_points_workspace_bytes(B, H, W) bytes, 4-byte aligned; ONE workspace serves one pair of calls at a time.
 * LA3D_ERR_ARG before any launch: a bad struct_size, both or neither of mask / mask_bits, both or neither of depth / depth16, a bad
 *   la3d_depth16, frame_width outside [0, W], negative sizes or strides, strides below a plane, NULL K / workspace / outputs with work to
 *   do (points may be NULL with capacity 0: every cloud is empty or has no room, no row is written), misaligned mask_bits / bits_offsets / frames / depth, frames with u8 masks or without image_index, bits_offsets without
 *   frames.  LA3D_ERR_UNSUPPORTED: W > 65536 (a row must fit a band's bit image in LDS), H * W >= 2^31, B x bands >= 2^31. */
#define LA3D_CLOUD_OK 0
#define LA3D_CLOUD_NO_ROOM 1
#define LA3D_CLOUD_MISMATCH 2
typedef struct la3d_cloud_args {
  int32_t struct_size;                                   /* sizeof(la3d_cloud_args) of the caller */
  int32_t B, H, W;
  int32_t frame_width;                                   /* 0 = W */
  int32_t k_stride;
  const float* depth; int64_t depth_plane_stride;        /* float32 planes, or NULL with depth16 */
  const la3d_depth16* depth16;                           /* HOST block, read before the call returns */
  const int32_t* image_index;                            /* dev [B] | NULL (frames: required) */
  const uint8_t* mask; int64_t mask_plane_stride;        /* u8 planes | NULL */
  const uint32_t* mask_bits; int64_t bits_plane_stride;  /* bit planes | NULL */
  const double* K;
  const int32_t* sample_idx;                             /* dev [B][500] | NULL */
  const la3d_frame* frames; int32_t P;                   /* dev [P] | NULL: the frames form */
  int32_t out_is_f64;                                    /* points: f64 (the reference's dtype) when != 0, else f32 */
  const int64_t* bits_offsets;                           /* dev [B], frames form */
  int32_t* counts;                                       /* dev [B]: first stage */
  int64_t* offsets;                                      /* dev [B+1]: written by the first stage, read by the second */
  void* points;                                          /* dev [capacity][3] */
  int32_t* pixels;                                       /* dev [capacity] | NULL */
  int32_t* status;                                       /* dev [B] */
  int64_t capacity;                                      /* rows of points / pixels */
  void* workspace; void* stream;
} la3d_cloud_args;
size_t la3d_instance_points_workspace_bytes(int B, int H, int W);   /* host, no device; 0 for B, H or W <= 0 */
int la3d_instance_point_offsets(const la3d_cloud_args* args);
int la3d_gather_instance_points(const la3d_cloud_args* args);

/* Host-pointer single calls (round 5): the reference's own calling pattern is one object / one image per call on NumPy arrays.
 * One C call = upload + kernel + download, synchronous, on a private stream of the calling thread; the staging memory (pinned and
 * device-mapped for the cloud, device scratch for the frame) belongs to the library, is per thread and per device, grows on demand
 * and is kept until la3d_host_release() / process exit.  ALL pointers are HOST pointers.
 *
 * la3d_estimate_bbox_host replaces estimate_bbox(in_pc, cat_name, ground_equ, method) for ONE cloud — reference
 * src/util_3dbox.py:106-178, call site :273-278.  points f64 [n][3] (the caller has already drawn its 500 rows when n > 500,
 * exactly where the reference draws them, :123-125); ground4 NULL or a NaN first entry = "ground_equ is None"; out39 / aux4 /
 * status as la3d_fit_points writes them (aux4 may be NULL).  PCA: the arithmetic of la3d_fit_points with
 * LA3D_HINT_SMALL_CLOUDS, bit for bit.
 *
 * la3d_unproject_host replaces depth_to_points(depth[None], K) for ONE frame — reference src/util.py:52-75, call site
 * src/batch_scripts/depth.py:154: depth f32 [H][W] -> out f64 / f32 [H][W][3], same arithmetic as la3d_unproject. */
int la3d_estimate_bbox_host(const double* points, int64_t n, const double* ground4, int method, double* out39, double* aux4,
                            int32_t* status);
int la3d_unproject_host(const float* depth, const double* K9, const double* Rt12, int H, int W, void* out, int out_is_f64);
void la3d_host_release(void);   /* frees the calling thread's staging memory and stream (optional) */

/* The reference's per-IMAGE pattern as one foreign call (round 5): the annotations of an image as run lengths or polygon parts ->
 * decode + the reference's keep rule + fit (la3d_fit_instances_ex with the filter fields) -> records.  `args` is a la3d_fit_args in which
 * `depth` is a DEVICE pointer (the image's depth plane(s), resident) and EVERY OTHER pointer is a HOST pointer: rle_counts / rle_offsets
 * or poly_xy / ring_offsets / inst_rings, K, image_index, ground, area_hint in; out / status / aux / stats out.  mask, sample_idx, proj
 * and workspace must be NULL / are ignored (the library uses the calling thread's staging memory).
 * `stream` = the stream the depth plane(s) were PRODUCED on (NULL = the legacy default stream): the call's upload, fit and completion
 * flag are enqueued on THAT stream, behind everything it holds, so a depth map a model / an upload / la3d_pad_rows has only enqueued
 * there is complete before the fit reads it.  Depth produced on any other stream must be complete before the call.  The depth must
 * live on the CURRENT device of the calling thread (hipSetDevice before the call).
 * Synchronous.  Replaces read_bounding_boxes_segmentations + the per-object fit for one image: src/util.py:336-383, util_3dbox.py:250-281. */
int la3d_fit_annotations_host(const la3d_fit_args* args);

/* The reference's per-scene box file from packed records, on the HOST (round 5; labelany3d_amd/csrc/la3d_json.cpp): the text
 * json.dump([{"obj_id", "category_name", "center_cam", "R_cam", "dimensions", "bbox3D_cam"}, ...], f) writes - reference
 * src/util_3dbox.py:283-292 - byte for byte (floats as float.__repr__ prints them), for S scenes in one call, without a Python
 * object per record.  records host f64 [*][39]; scene s owns entries [scene_off[s], scene_off[s+1]) of rows (record row) / obj_ids /
 * name_ids (index into names_json: UTF-8, already JSON-escaped and quoted); out: host buffer of `cap` bytes
 * (la3d_3dbbox_json_bound(entries, total name bytes, S)); text_off [S+1]: scene s's text = out[text_off[s] .. text_off[s+1]).
 * Returns the bytes written, -1 if cap is too small or an argument is missing. */
int64_t la3d_3dbbox_json_bound(int64_t n, int64_t name_bytes, int64_t S);
int64_t la3d_format_3dbbox_json(const double* records, const int64_t* rows, const int32_t* obj_ids, const int32_t* name_ids,
                                const int64_t* scene_off, int32_t S, const char* const* names_json, char* out, int64_t cap,
                                int64_t* text_off);

/* Host-side staging helper (no device work): n pageable source planes of bytes_each bytes -> consecutive slots of dst (a pinned
 * buffer), copied by `threads` native threads in one call (labelany3d_amd/fit_scenes.py: the depth_map.npy planes of a batch,
 * reference src/batch_scripts/whole.py:63-67).  0 on success, -1 on a bad argument. */
int la3d_gather_planes_host(const void* const* src, int64_t n, int64_t bytes_each, void* dst, int threads);

/* Host-side helper exported for tests: float64 -> float16 (round-to-nearest-even, as NumPy's
 * astype(float16), reference src/util_3dbox.py:165) -> float64, the same routine the kernels use. */
double la3d_f16_round_host(double x);

#ifdef __cplusplus
}
#endif
#endif /* LA3D_H */
