"""labelany3d_amd — MI355X-native (gfx950) implementation of LabelAny3D's geometric hot path:
depth back-projection (reference src/util.py:52-75) and oriented 3D box fitting (reference
src/util_3dbox.py:106-178), behind the reference's own function signatures.

    from labelany3d_amd import fit_instances            # batched: depth + masks -> (B,39) boxes on the GPU
    from labelany3d_amd.util_3dbox import estimate_bbox # drop-in scalar signature
    from labelany3d_amd.util import depth_to_points

All compute goes through libla3d.so (hand-written HIP, C-ABI in include/la3d.h); there is no CPU path.
"""
from ._lib import AUX, NSAMPLE, REC, La3dError  # noqa: F401
from .assign import AssignPlan, Assignment, BoxIou, assign_batch, assign_overlap, assign_plan, iou2d_groups, match_boxes, match_masks  # noqa: F401
from .batched import (Depth16, InstanceFitter, draw_sample_idx, fit_instances, fit_points, mask_counts, pad_depth_rows, padded_width, unpack_boxes,  # noqa: F401
                      unproject)
from .bits import (DepthGateStats, MaskBits, crop_placement, depth_gate_stats, fit_instances_bits, gate_depth_bits, mask_stats_bits, pack_crop_bits, pack_logits_bits, pack_mask_bits, pack_poly_bits,  # noqa: F401
                   pack_rle_bits, unpack_mask_bits)
from .clouds import InstancePoints, instance_points, instance_points_frames  # noqa: F401
from .components import (components_bits, components_bits_frames, components_stats, components_stats_frames, drop_islands_bits,  # noqa: F401
                         drop_islands_bits_frames, largest_component_bits, largest_component_bits_frames)
from .consumers import correspondences_to_world, hungarian_matching, iou2d_matrix, project_boxes, unproject_matches  # noqa: F401
from .depth16 import pack_depth16, unpack_depth16  # noqa: F401
from .depth_align import (PlaneFit, RansacScale, align_apply, align_depth, align_depth_batch, align_select, align_select_batch, depth_match_transform,  # noqa: F401
                          ground_planes, masked_ratio_median, plane_ransac_batch, plane_select_batch, ransac_scale_batch, ransac_subsets)
from .frames import (FrameBits, FrameGrid, PackedFrames, PackedFrames16, PackedLabels, PackedMasks, fit_instances_frames, fit_instances_frames_bits,  # noqa: F401
                     fit_instances_frames_labels, fit_instances_frames_masks, frame_bits_offsets, pack_crop_bits_frames, pack_frames,
                     pack_label_bits_frames, pack_label_frames, pack_mask_bits_frames, pack_mask_frames, pack_poly_bits_frames, pack_rle_bits_frames, scaled_frames)
from .labels import LabelBits, fit_instances_labels, label_instances, pack_label_bits  # noqa: F401
from .masks import annotation_areas, filter_annotations, fit_annotations, fit_annotations_all, fit_instances_ex, fit_instances_poly, fit_instances_rle, keep_instances, mask_stats, mask_stats_poly, mask_stats_rle, poly_decode, rle_decode, segmentations_to_masks  # noqa: F401
from .morph import (bits_rects, bits_rects_frames, crop_params, depth_gate_stats_frames, gate_depth_bits_frames, open_bits, open_bits_frames, select_crops,  # noqa: F401
                    select_crops_frames)
from .options import scheduling  # noqa: F401
from .overlap import MaskOverlap, OverlapPlan, mask_iou, mask_nms, mask_overlap, mask_overlap_plan  # noqa: F401
from .pipeline import fit_batches  # noqa: F401
from .rle_encode import RleRuns, rle_encode, rle_encode_bits, rle_encode_bits_frames, rle_objects, rle_to_string  # noqa: F401
from .segm import pack_polygons, pack_rle, rle_from_string  # noqa: F401

__all__ = ["ground_planes", "plane_select_batch", "plane_ransac_batch", "PlaneFit", "gate_depth_bits", "depth_gate_stats", "DepthGateStats", "gate_depth_bits_frames", "depth_gate_stats_frames", "Assignment", "AssignPlan", "BoxIou", "assign_batch", "assign_overlap", "assign_plan", "iou2d_groups", "match_boxes", "match_masks", "components_bits", "components_stats", "largest_component_bits", "drop_islands_bits", "components_bits_frames", "components_stats_frames", "largest_component_bits_frames", "drop_islands_bits_frames", "MaskOverlap", "OverlapPlan", "mask_overlap", "mask_overlap_plan", "mask_iou", "mask_nms", "open_bits", "bits_rects", "crop_params", "select_crops", "FrameGrid", "scaled_frames", "open_bits_frames", "bits_rects_frames", "select_crops_frames", "RleRuns", "rle_encode", "rle_encode_bits", "rle_encode_bits_frames", "rle_objects", "rle_to_string", "crop_placement", "pack_crop_bits", "pack_crop_bits_frames", "pack_rle_bits", "pack_poly_bits", "pack_rle_bits_frames", "pack_poly_bits_frames", "InstancePoints", "instance_points", "instance_points_frames", "PackedMasks", "pack_mask_frames", "pack_mask_bits_frames", "fit_instances_frames_masks", "FrameBits", "PackedLabels", "pack_label_frames", "pack_label_bits_frames", "frame_bits_offsets", "fit_instances_frames_bits",
           "fit_instances_frames_labels", "LabelBits", "pack_label_bits", "fit_instances_labels", "label_instances", "Depth16", "pack_depth16", "unpack_depth16", "fit_instances_frames", "pack_frames", "PackedFrames", "PackedFrames16", "fit_instances_bits", "pack_mask_bits", "pack_logits_bits", "unpack_mask_bits", "mask_stats_bits", "MaskBits", "fit_instances_ex", "fit_annotations", "fit_annotations_all", "annotation_areas", "correspondences_to_world", "fit_batches", "scheduling", "align_depth", "align_depth_batch", "ransac_scale_batch", "ransac_subsets", "RansacScale", "align_select", "align_select_batch", "align_apply", "depth_match_transform", "fit_instances_poly", "pack_polygons", "poly_decode", "mask_stats_poly", "segmentations_to_masks", "unproject_matches", "masked_ratio_median", "project_boxes", "iou2d_matrix", "hungarian_matching", "fit_instances_rle", "rle_decode", "filter_annotations", "mask_stats", "mask_stats_rle", "keep_instances", "pack_rle", "pad_depth_rows", "padded_width", "rle_from_string","fit_instances", "fit_points", "mask_counts", "unproject", "draw_sample_idx", "unpack_boxes",
           "InstanceFitter", "La3dError", "REC", "AUX", "NSAMPLE"]
