"""ctypes binding of libla3d.so (C-ABI in include/la3d.h).  No CPU fallback: if the HIP library
is missing, importing this module raises — the product path is the GPU path."""
from __future__ import annotations

import ctypes as C
import os

from ._build import HERE, INCLUDE, LIB, ROOT, SOURCES, build  # noqa: F401

REC, AUX, NSAMPLE = 39, 4, 500
BOX_OK, BOX_EMPTY, BOX_BAD_GROUND, BOX_TOO_FEW, BOX_NONFINITE, BOX_UNSUPPORTED, BOX_FILTERED = 0, 1, 2, 3, 4, 5, 6
METHOD_PCA, METHOD_CONVEX_HULL = 0, 1
HINT_SMALL_CLOUDS = 0x100
HINT_HULL_512 = 0x200
ERR_UNSUPPORTED = -2
BITS_HEIGHT_ROWS, BITS_HEIGHT_SPAN = 0, 1          # flags of la3d_fit_instances_bits: the height rule of the fused filter
DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2        # la3d_pack_logits_bits
DTYPE_U16 = 3                                     # la3d_depth16 (with DTYPE_F16): uint16 x scale depth planes
LABEL_U8, LABEL_U16, LABEL_I32, LABEL_RGB8 = 0, 1, 2, 3   # la3d_pack_label_bits: the element of a label map
DEPTH_ZERO_IS_HOLE = 1                            # la3d_depth16.flags (U16): a stored 0 is a hole (NaN)

class FitArgs(C.Structure):
    """``la3d_fit_args`` of include/la3d.h (argument block of la3d_fit_instances_ex); field order is the header's."""
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("depth", C.c_void_p), ("depth_plane_stride", C.c_int64), ("image_index", C.c_void_p),
                ("mask", C.c_void_p),
                ("rle_counts", C.c_void_p), ("rle_offsets", C.c_void_p),
                ("poly_xy", C.c_void_p), ("ring_offsets", C.c_void_p), ("inst_rings", C.c_void_p),
                ("K", C.c_void_p), ("k_stride", C.c_int32),
                ("filter_boundary", C.c_int32), ("filter_min_area", C.c_int32), ("filter_max_edge", C.c_int32),
                ("ground", C.c_void_p), ("sample_idx", C.c_void_p),
                ("stats", C.c_void_p),
                ("proj", C.c_void_p), ("image_width", C.c_double), ("image_height", C.c_double),
                ("out", C.c_void_p), ("status", C.c_void_p), ("aux", C.c_void_p),
                ("workspace", C.c_void_p), ("stream", C.c_void_p),
                ("area_hint", C.c_void_p),
                ("opt_engine", C.c_int32), ("opt_launch_order", C.c_int32), ("opt_build", C.c_int32), ("frame_width", C.c_int32),
                ("method", C.c_int32)]


class Depth16Block(C.Structure):
    """``la3d_depth16`` of include/la3d.h: the 16-bit depth planes of la3d_fit_instances_depth16 (32 bytes)."""
    _fields_ = [("struct_size", C.c_int32), ("dtype", C.c_int32), ("planes", C.c_void_p), ("plane_stride", C.c_int64),
                ("scale", C.c_float), ("flags", C.c_int32)]


class Frame(C.Structure):
    """``la3d_frame`` of include/la3d.h: one row per image of a frames call (la3d_fit_instances_frames)."""
    _fields_ = [("depth_offset", C.c_int64), ("H", C.c_int32), ("W", C.c_int32), ("frame_width", C.c_int32), ("reserved", C.c_int32)]


class CloudArgs(C.Structure):
    """``la3d_cloud_args`` of include/la3d.h (argument block of la3d_instance_point_offsets / la3d_gather_instance_points, 192 bytes);
    field order is the header's."""
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("frame_width", C.c_int32), ("k_stride", C.c_int32),
                ("depth", C.c_void_p), ("depth_plane_stride", C.c_int64), ("depth16", C.POINTER(Depth16Block)),
                ("image_index", C.c_void_p),
                ("mask", C.c_void_p), ("mask_plane_stride", C.c_int64), ("mask_bits", C.c_void_p), ("bits_plane_stride", C.c_int64),
                ("K", C.c_void_p), ("sample_idx", C.c_void_p),
                ("frames", C.c_void_p), ("P", C.c_int32), ("out_is_f64", C.c_int32), ("bits_offsets", C.c_void_p),
                ("counts", C.c_void_p), ("offsets", C.c_void_p), ("points", C.c_void_p), ("pixels", C.c_void_p), ("status", C.c_void_p),
                ("capacity", C.c_int64), ("workspace", C.c_void_p), ("stream", C.c_void_p)]


class AlignRansacArgs(C.Structure):
    """``la3d_align_ransac_args`` of include/la3d.h (argument block of la3d_align_ransac_batch, 136 bytes); field order is the header's."""
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("n", C.c_int64),
                ("relative_sel", C.c_void_p), ("metric_sel", C.c_void_p), ("counts", C.c_void_p),
                ("min_samples", C.c_double), ("stop_probability", C.c_double),
                ("max_trials", C.c_int32), ("m_cap", C.c_int32), ("subsets", C.c_void_p), ("seed", C.c_uint64),
                ("coef", C.c_void_p), ("n_inliers", C.c_void_p), ("n_trials", C.c_void_p), ("best_trial", C.c_void_p),
                ("status", C.c_void_p), ("workspace", C.c_void_p), ("stream", C.c_void_p)]


ALIGN_OK, ALIGN_EMPTY, ALIGN_FAILED = 0, 1, 2       # status of la3d_align_ransac_batch
ALIGN_RANSAC_MAX_N, ALIGN_RANSAC_MAX_TRIALS = 1 << 24, 1024

class PlaneSelectArgs(C.Structure):
    """``la3d_plane_select_args`` of include/la3d.h (argument block of la3d_plane_select_batch, 112 bytes); field order is the header's."""
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("step", C.c_int32), ("k_stride", C.c_int32), ("near_depth", C.c_float), ("far_depth", C.c_float),
                ("depth", C.c_void_p), ("K", C.c_void_p), ("candidates", C.c_void_p), ("cand_plane_stride", C.c_int64),
                ("cand_width", C.c_int32), ("reserved", C.c_int32),
                ("points", C.c_void_p), ("pixel", C.c_void_p), ("counts", C.c_void_p), ("workspace", C.c_void_p), ("stream", C.c_void_p)]


class PlaneRansacArgs(C.Structure):
    """``la3d_plane_ransac_args`` of include/la3d.h (argument block of la3d_plane_ransac_batch, 152 bytes); field order is the header's."""
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("n", C.c_int64),
                ("points", C.c_void_p), ("counts", C.c_void_p),
                ("thr_abs", C.c_double), ("thr_rel", C.c_double), ("cos2_tilt", C.c_double),
                ("max_trials", C.c_int32), ("min_inliers", C.c_int32), ("subsets", C.c_void_p), ("seed", C.c_uint64),
                ("plane", C.c_void_p), ("k_trial", C.c_void_p), ("n_inliers", C.c_void_p), ("best_trial", C.c_void_p),
                ("rms", C.c_void_p), ("status", C.c_void_p), ("inliers", C.c_void_p), ("workspace", C.c_void_p), ("stream", C.c_void_p)]


PLANE_OK, PLANE_TOO_FEW, PLANE_FAILED, PLANE_BROKEN = 0, 1, 2, 3   # status of la3d_plane_ransac_batch
PLANE_MAX_N, PLANE_MAX_TRIALS, PLANE_SEGMENT = 1 << 24, 1024, 1024

CLOUD_OK, CLOUD_NO_ROOM, CLOUD_MISMATCH = 0, 1, 2  # status of la3d_gather_instance_points (5 = BOX_UNSUPPORTED: a refused frames row)


class RleEncodeArgs(C.Structure):
    """``la3d_rle_encode_args`` of include/la3d.h (argument block of la3d_rle_encode_offsets / la3d_rle_encode, 120 bytes); field order
    is the header's."""
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("frame_width", C.c_int32), ("P", C.c_int32),
                ("mask_bits", C.c_void_p), ("bits_plane_stride", C.c_int64),
                ("frames", C.c_void_p), ("image_index", C.c_void_p), ("bits_offsets", C.c_void_p),
                ("runs", C.c_void_p), ("offsets", C.c_void_p), ("counts", C.c_void_p), ("status", C.c_void_p),
                ("capacity", C.c_int64), ("workspace", C.c_void_p), ("stream", C.c_void_p)]


RLE_OK, RLE_NO_ROOM, RLE_MISMATCH = 0, 1, 2        # status of la3d_rle_encode (5 = BOX_UNSUPPORTED: a refused frames row)


class ComponentsArgs(C.Structure):
    """``la3d_components_args`` of include/la3d.h (argument block of la3d_components_bits, 104 bytes); field order is the header's."""
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("frame_width", C.c_int32), ("connectivity", C.c_int32), ("min_area", C.c_int32), ("largest", C.c_int32),
                ("max_runs", C.c_int32), ("max_components", C.c_int32),
                ("mask_bits", C.c_void_p), ("bits_plane_stride", C.c_int64), ("out_bits", C.c_void_p), ("out_plane_stride", C.c_int64),
                ("stats", C.c_void_p), ("components", C.c_void_p), ("workspace", C.c_void_p), ("stream", C.c_void_p)]


class ComponentsFramesArgs(C.Structure):
    """``la3d_components_frames_args`` of include/la3d.h (argument block of la3d_components_bits_frames, 144 bytes); field order is
    the header's."""
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("P", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("connectivity", C.c_int32), ("min_area", C.c_int32), ("largest", C.c_int32), ("max_runs", C.c_int32),
                ("max_components", C.c_int32), ("reserved", C.c_int32 * 2),
                ("bits", C.c_void_p), ("bits_words", C.c_int64), ("bits_offsets", C.c_void_p),
                ("frames", C.c_void_p), ("image_index", C.c_void_p),
                ("out_bits", C.c_void_p), ("out_words", C.c_int64), ("out_offsets", C.c_void_p),
                ("stats", C.c_void_p), ("components", C.c_void_p), ("workspace", C.c_void_p), ("stream", C.c_void_p)]


COMPONENTS_MAX_RUNS = 524288                      # la3d_components_bits: the largest max_runs (a plane of 2^20 pixels has no more)


class OverlapTile(C.Structure):
    """``la3d_overlap_tile`` of include/la3d.h: one row of the tile table of la3d_mask_overlap_plan (64 bytes)."""
    _fields_ = [("g", C.c_int32), ("i0", C.c_int32), ("j0", C.c_int32), ("ni", C.c_int32), ("nj", C.c_int32),
                ("row_a", C.c_int32), ("row_b", C.c_int32), ("w0", C.c_int32), ("w1", C.c_int32), ("nw", C.c_int32),
                ("chunk", C.c_int32), ("nchunks", C.c_int32), ("nb", C.c_int32), ("flags", C.c_int32), ("out0", C.c_int64)]


class MaskOverlapArgs(C.Structure):
    """``la3d_mask_overlap_args`` of include/la3d.h (argument block of la3d_mask_overlap, 208 bytes); field order is the header's."""
    _fields_ = [("struct_size", C.c_int32), ("G", C.c_int32), ("kind", C.c_int32), ("P", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("rows_a", C.c_int64), ("rows_b", C.c_int64),
                ("a_bits", C.c_void_p), ("b_bits", C.c_void_p), ("a_stride", C.c_int64), ("b_stride", C.c_int64), ("nwords", C.c_int64),
                ("frames", C.c_void_p), ("a_offsets", C.c_void_p), ("b_offsets", C.c_void_p),
                ("a_image_index", C.c_void_p), ("b_image_index", C.c_void_p), ("a_words", C.c_int64), ("b_words", C.c_int64),
                ("tiles", C.c_void_p), ("ntiles", C.c_int64), ("npairs", C.c_int64),
                ("inter", C.c_void_p), ("area_a", C.c_void_p), ("area_b", C.c_void_p), ("iou", C.c_void_p),
                ("workspace", C.c_void_p), ("stream", C.c_void_p)]


class MaskNmsArgs(C.Structure):
    """``la3d_mask_nms_args`` of include/la3d.h (argument block of la3d_mask_nms, 96 bytes); field order is the header's."""
    _fields_ = [("struct_size", C.c_int32), ("G", C.c_int32), ("kind", C.c_int32), ("reserved", C.c_int32), ("B", C.c_int64),
                ("inter", C.c_void_p), ("area", C.c_void_p), ("offsets", C.c_void_p), ("row_offsets", C.c_void_p),
                ("order", C.c_void_p), ("labels", C.c_void_p), ("thr", C.c_double), ("keep", C.c_void_p), ("stream", C.c_void_p)]


class AssignArgs(C.Structure):
    """``la3d_assign_args`` of include/la3d.h (argument block of la3d_assign, 112 bytes); field order is the header's."""
    _fields_ = [("struct_size", C.c_int32), ("G", C.c_int32), ("cost", C.c_void_p), ("cost_dtype", C.c_int32), ("reserved0", C.c_int32),
                ("ncost", C.c_int64), ("offsets", C.c_void_p), ("row_offsets_a", C.c_void_p), ("row_offsets_b", C.c_void_p),
                ("rows_a", C.c_int64), ("rows_b", C.c_int64), ("maximize", C.c_int32), ("reserved1", C.c_int32),
                ("col_of_row", C.c_void_p), ("row_of_col", C.c_void_p), ("status", C.c_void_p), ("stream", C.c_void_p)]


class IouGroupsArgs(C.Structure):
    """``la3d_iou_groups_args`` of include/la3d.h (argument block of la3d_iou_matrix_groups, 88 bytes); field order is the header's."""
    _fields_ = [("struct_size", C.c_int32), ("G", C.c_int32), ("boxes_a", C.c_void_p), ("boxes_b", C.c_void_p),
                ("rows_a", C.c_int64), ("rows_b", C.c_int64), ("row_offsets_a", C.c_void_p), ("row_offsets_b", C.c_void_p),
                ("offsets", C.c_void_p), ("npairs", C.c_int64), ("out", C.c_void_p), ("stream", C.c_void_p)]


class DepthGateArgs(C.Structure):
    """``la3d_depth_gate_args`` of include/la3d.h (argument block of la3d_depth_gate_bits, 120 bytes); field order is the header's."""
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("frame_width", C.c_int32),
                ("k", C.c_float), ("min_band", C.c_float), ("near", C.c_float), ("far", C.c_float), ("reserved", C.c_int32),
                ("depth", C.c_void_p), ("depth_plane_stride", C.c_int64), ("image_index", C.c_void_p),
                ("mask_bits", C.c_void_p), ("bits_plane_stride", C.c_int64), ("out_bits", C.c_void_p), ("out_plane_stride", C.c_int64),
                ("counts", C.c_void_p), ("levels", C.c_void_p), ("stream", C.c_void_p)]


class DepthGateFramesArgs(C.Structure):
    """``la3d_depth_gate_frames_args`` of include/la3d.h (argument block of la3d_depth_gate_bits_frames, 152 bytes); field order is the
    header's."""
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("P", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("k", C.c_float), ("min_band", C.c_float), ("near", C.c_float), ("far", C.c_float), ("reserved", C.c_int32),
                ("depth", C.c_void_p), ("depth16", C.POINTER(Depth16Block)), ("depth_elems", C.c_int64),
                ("frames", C.c_void_p), ("image_index", C.c_void_p),
                ("bits", C.c_void_p), ("bits_words", C.c_int64), ("bits_offsets", C.c_void_p),
                ("out_bits", C.c_void_p), ("out_words", C.c_int64), ("out_offsets", C.c_void_p),
                ("counts", C.c_void_p), ("levels", C.c_void_p), ("stream", C.c_void_p)]


DEPTH_GATE_MAX_PIXELS = 857728                                         # la3d_depth_gate_bits[_frames]: the stored pixels of a frame (of the bounds) its LDS layout holds

ASSIGN_F64, ASSIGN_I32 = 0, 1                                          # la3d_assign_args.cost_dtype
ASSIGN_MAX_N, ASSIGN_STAGE_MAX = 256, 2048                             # rows / columns of a group; elements staged in LDS
ASSIGN_OK, ASSIGN_INVALID, ASSIGN_INFEASIBLE, ASSIGN_TOO_LARGE, ASSIGN_BROKEN = 0, 1, 2, 3, 4   # status of a group
OVERLAP_NONE, OVERLAP_IOU, OVERLAP_IOM, OVERLAP_IOA = 0, 1, 2, 3      # la3d_mask_overlap_args.kind
OVERLAP_MIRROR, OVERLAP_AREA_A, OVERLAP_AREA_B = 1, 2, 4              # la3d_overlap_tile.flags
OVERLAP_TILE, OVERLAP_STEP = 8, 1024                                   # planes per side of a tile; words a chunk is a multiple of

_SIGS = {
    "la3d_plane_select_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "la3d_plane_select_batch": (C.c_int, [C.POINTER(PlaneSelectArgs)]),
    "la3d_plane_ransac_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int]),
    "la3d_plane_ransac_batch": (C.c_int, [C.POINTER(PlaneRansacArgs)]),
    "la3d_depth_gate_bits": (C.c_int, [C.POINTER(DepthGateArgs)]),
    "la3d_depth_gate_bits_frames": (C.c_int, [C.POINTER(DepthGateFramesArgs)]),
    "la3d_mask_overlap_plan": (C.c_int64, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "la3d_mask_overlap_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "la3d_mask_overlap": (C.c_int, [C.POINTER(MaskOverlapArgs)]),
    "la3d_mask_nms": (C.c_int, [C.POINTER(MaskNmsArgs)]),
    "la3d_assign": (C.c_int, [C.POINTER(AssignArgs)]),
    "la3d_iou_matrix_groups": (C.c_int, [C.POINTER(IouGroupsArgs)]),
    "la3d_components_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "la3d_components_bits": (C.c_int, [C.POINTER(ComponentsArgs)]),
    "la3d_components_bits_frames": (C.c_int, [C.POINTER(ComponentsFramesArgs)]),
    "la3d_open_bits_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "la3d_open_bits": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_open_bits_frames_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "la3d_open_bits_frames": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                        C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_rle_encode_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "la3d_rle_encode_offsets": (C.c_int, [C.POINTER(RleEncodeArgs)]),
    "la3d_rle_encode": (C.c_int, [C.POINTER(RleEncodeArgs)]),
    "la3d_rle_to_string_host": (C.c_int64, [C.c_void_p, C.c_int64, C.c_char_p, C.c_int64]),
    "la3d_instance_points_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "la3d_instance_point_offsets": (C.c_int, [C.POINTER(CloudArgs)]),
    "la3d_gather_instance_points": (C.c_int, [C.POINTER(CloudArgs)]),
    "la3d_fit_instances_ex": (C.c_int, [C.POINTER(FitArgs)]),
    "la3d_fit_instances_frames": (C.c_int, [C.POINTER(FitArgs), C.c_void_p, C.c_int32]),
    "la3d_fit_instances_frames_depth16": (C.c_int, [C.POINTER(FitArgs), C.POINTER(Depth16Block), C.c_void_p, C.c_int32]),
    "la3d_fit_instances_frames_bits": (C.c_int, [C.POINTER(FitArgs), C.POINTER(Depth16Block), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                                 C.c_int32]),
    "la3d_pack_label_bits_frames": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_pack_mask_bits_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_pack_logits_bits_frames": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_pack_rle_bits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p]),
    "la3d_pack_poly_bits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p]),
    "la3d_pack_rle_bits_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_pack_poly_bits_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p,
                                             C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_pack_crop_bits": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "la3d_pack_crop_bits_frames": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int32,
                                             C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_fit_workspace_bytes": (C.c_size_t, [C.POINTER(FitArgs)]),
    "la3d_fit_instances_bits": (C.c_int, [C.POINTER(FitArgs), C.c_void_p, C.c_int64, C.c_int32]),
    "la3d_fit_instances_depth16": (C.c_int, [C.POINTER(FitArgs), C.POINTER(Depth16Block), C.c_void_p, C.c_int64, C.c_int32]),
    "la3d_pack_depth16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int64,
                                    C.c_void_p]),
    "la3d_unpack_depth16": (C.c_int, [C.POINTER(Depth16Block), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "la3d_mask_bits_words": (C.c_size_t, [C.c_int, C.c_int]),
    "la3d_pack_mask_bits": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "la3d_pack_logits_bits": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_int64, C.c_void_p]),
    "la3d_pack_label_bits": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "la3d_unpack_mask_bits": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "la3d_mask_stats_bits": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "la3d_version": (C.c_int, []),
    "la3d_last_error": (C.c_char_p, []),
    "la3d_unproject": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int,
                                 C.c_void_p, C.c_int, C.c_void_p]),
    "la3d_unproject_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_int, C.c_void_p]),
    "la3d_mask_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "la3d_pad_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "la3d_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "la3d_fit_instances": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_fit_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_f16_round_host": (C.c_double, [C.c_double]),
    "la3d_fit_instances_rle": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_fit_instances_poly": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_fit_instances_rle_filtered": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_fit_instances_poly_filtered": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_poly_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "la3d_mask_stats_poly": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p]),
    "la3d_rle_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "la3d_mask_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "la3d_mask_stats_rle": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "la3d_masked_ratio_median": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_align_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "la3d_align_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "la3d_align_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "la3d_align_select_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_align_ransac_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int]),
    "la3d_align_ransac_batch": (C.c_int, [C.POINTER(AlignRansacArgs)]),
    "la3d_align_ransac_subsets": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]),
    "la3d_align_apply_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_float,
                                         C.c_void_p, C.c_void_p]),
    "la3d_unproject_matches": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double,
                                         C.c_double, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "la3d_project_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_double, C.c_double,
                                     C.c_void_p, C.c_void_p]),
    "la3d_iou_matrix": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "la3d_build_info": (C.c_char_p, []),
    "la3d_rle_from_string_host": (C.c_int, [C.c_char_p, C.c_int64, C.POINTER(C.c_int32), C.c_int]),
    "la3d_estimate_bbox_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "la3d_unproject_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "la3d_host_release": (None, []),
    "la3d_fit_annotations_host": (C.c_int, [C.POINTER(FitArgs)]),
    "la3d_gather_planes_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int]),
    "la3d_3dbbox_json_bound": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    "la3d_format_3dbbox_json": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_int64, C.c_void_p]),
}

EXPORTS = tuple(_SIGS)


def _refresh_if_stale() -> None:
    """The library carries the hash of the sources it was compiled from (la3d_build_info).  A library that travelled with a
    snapshot but was built from OTHER sources than the tree's is rebuilt here, once, under a file lock (several test processes
    may import at the same time) - when hipcc is there; otherwise it is used as it is, loudly.  LA3D_NO_AUTOBUILD=1 switches
    the rebuild off (the library is then loaded as it is; bench.py's `build.lib_built_from_tree` tells)."""
    import sys

    from . import _build
    try:
        have = _build.embedded_info(LIB)
        if have is not None and have[0] == _build.source_sha256():
            return
        if os.environ.get("LA3D_NO_AUTOBUILD") == "1" or os.environ.get("LA3D_LIB"):
            return
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not os.path.exists(hipcc):
            print(f"labelany3d_amd: {LIB} was NOT built from the sources in this tree and there is no hipcc to rebuild it", file=sys.stderr)
            return
        import fcntl
        with open(LIB + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            have = _build.embedded_info(LIB)                    # (another process may have rebuilt it meanwhile)
            if have is None or have[0] != _build.source_sha256():
                print(f"labelany3d_amd: {os.path.basename(LIB)} is stale (built from other sources): rebuilding for gfx950 ...", file=sys.stderr)
                _build.build(force=True)
    except Exception as e:  # noqa: BLE001 - never in the way of loading what is there
        print(f"labelany3d_amd: could not refresh {LIB}: {e!r}", file=sys.stderr)


def load() -> C.CDLL:
    if not os.path.exists(LIB):
        raise ImportError(
            f"{LIB} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(needs hipcc; cross-compiles gfx950 without a GPU). There is no CPU fallback."
        )
    _refresh_if_stale()
    # PyTorch bundles its own libamdhip64; load it FIRST so that libla3d.so binds to the same HIP runtime instance as the
    # tensors it is handed (loaded the other way round, the process ends up with two runtimes and the library's stream /
    # event calls fail with "no ROCm-capable device is detected")
    import torch  # noqa: F401

    lib = C.CDLL(LIB)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    return lib


lib = load()


class La3dError(RuntimeError):
    pass


_METHODS = {"pca": METHOD_PCA, "convex_hull": METHOD_CONVEX_HULL}


def method_code(method) -> int:
    """``method`` of the fit entries ("pca" | "convex_hull", the reference's estimate_bbox argument) -> LA3D_METHOD_*; anything else
    raises the reference's error (src/util_3dbox.py:151) - before any device work."""
    code = _METHODS.get(method) if isinstance(method, str) else None
    if code is None:
        raise ValueError(f"Unknown method: {method}. Use 'pca' or 'convex_hull'")
    return code


def fit_workspace_bytes(B: int, H: int, W: int, method: int = METHOD_PCA) -> int:
    """C-ABI ``la3d_fit_workspace_bytes`` for a call of B instances of H x W with the given LA3D_METHOD_* code."""
    a = FitArgs(struct_size=C.sizeof(FitArgs), B=B, H=H, W=W, method=method)
    return int(lib.la3d_fit_workspace_bytes(C.byref(a)))


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise La3dError(f"{what} failed ({rc}): {lib.la3d_last_error().decode()}")
