"""ctypes binding of lib3dal_hip.so (include/dal3.h). No torch math here: tensors are only a way
to own device memory (data_ptr) and to find the current HIP stream.

The library is REQUIRED: every eval-mode forward of the model classes goes through it, and
loading raises if it has not been built (python -c "import __graft_entry__ as g; g.build()" or
`make -C 3dal_pytorch_amd/csrc`). There is no CPU / eager fallback.
"""
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib3dal_hip.so")

OK, EINVAL, EWORKSPACE, EHIP = 0, -1, -2, -3
F32, BF16, F16, F16X3 = 0, 1, 2, 3
DTYPES = {"fp32": F32, "bf16": BF16, "fp16": F16, "f16x3": F16X3}
HEAD_INS_SEG, HEAD_STATIC_BOX_EST, HEAD_POINT_EMB, HEAD_BOX_EMB, HEAD_DYNAMIC_BOX_EST = range(5)
SAMPLER_DEVICE, SAMPLER_CHOICE = 0, 1
PHASE_SEG, PHASE_BOX, PHASE_ALL = 1, 2, 3

vp = C.c_void_p


class Layer(C.Structure):
    """dal3_layer"""
    _fields_ = [("weight", vp), ("bias", vp), ("bn_weight", vp), ("bn_bias", vp), ("bn_mean", vp),
                ("bn_var", vp), ("c_in", C.c_int32), ("c_out", C.c_int32)]


class PackItem(C.Structure):
    """dal3_tr_pack_item"""
    _fields_ = [("W", vp), ("ldw", C.c_int64), ("transpose_w", C.c_int32), ("c_out", C.c_int32), ("c_in", C.c_int32),
                ("mtb", C.c_int32), ("out", vp)]


class WgradPart(C.Structure):
    """dal3_tr_wgrad_part"""
    _fields_ = [("part", vp), ("n_slices", C.c_int64), ("n", C.c_int64), ("dW", vp)]


class BCN(C.Structure):
    """dal3_bcn"""
    _fields_ = [("data", vp), ("stride_b", C.c_int64), ("stride_c", C.c_int64), ("stride_n", C.c_int64),
                ("dtype", C.c_int32), ("flags", C.c_int32)]


class StaticArgs(C.Structure):
    """dal3_static_args"""
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("two_stage", C.c_int32), ("sampler", C.c_int32),
                ("dtype", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("item_offset", C.c_int64), ("pts", BCN),
                ("init_box", vp), ("bbox_gt", vp), ("choice", vp),
                ("w_ins_seg", vp), ("w_box_est_one", vp), ("w_box_est_two", vp),
                ("logits", vp), ("mask", vp),
                ("box_pred_one", vp), ("heading_residuals_one", vp), ("size_residuals_one", vp),
                ("center_one", vp), ("box_one", vp),
                ("box_pred_two", vp), ("heading_residuals_two", vp), ("size_residuals_two", vp),
                ("center_two", vp), ("heading_class_label_two", vp), ("heading_residuals_label_two", vp),
                ("boxes7", vp), ("counts", vp), ("obj_idx", vp),
                ("workspace", vp), ("workspace_bytes", C.c_size_t)]


class DynamicArgs(C.Structure):
    """dal3_dynamic_args"""
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("n_box", C.c_int32), ("sampler", C.c_int32),
                ("dtype", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("item_offset", C.c_int64), ("pts", BCN), ("box", BCN),
                ("init_box8", vp), ("choice", vp),
                ("w_ins_seg", vp), ("w_point_emb", vp), ("w_box_emb", vp), ("w_box_est", vp),
                ("logits", vp), ("mask", vp), ("embedding", vp), ("box_pred", vp),
                ("heading_residuals", vp), ("size_residuals", vp), ("boxes7", vp),
                ("counts", vp), ("obj_idx", vp),
                ("workspace", vp), ("workspace_bytes", C.c_size_t)]


class BoxMetricAcc(C.Structure):
    """dal3_box_metric_acc (48 bytes)"""
    _fields_ = [("sum_iou_bev", C.c_double), ("sum_iou_3d", C.c_double), ("sum_loss", C.c_double),
                ("n_iou_3d_pass", C.c_uint64), ("n_seg_correct", C.c_uint64), ("n_items", C.c_uint64)]


class BoxMetricArgs(C.Structure):
    """dal3_box_metric_args"""
    _fields_ = [("B", C.c_int64), ("N", C.c_int64)] + [
        f for name in ("center", "heading_scores", "heading_residuals", "size_scores", "size_residuals", "center_label",
                       "heading_class_label", "heading_residual_label", "size_class_label", "size_residual_label")
        for f in ((name, vp), ("ld_" + name, C.c_int64))] + [
        ("f64_fields", C.c_int32), ("i32_fields", C.c_int32),
        ("logits", vp), ("logits_stride_b", C.c_int64), ("logits_stride_n", C.c_int64), ("logits_stride_c", C.c_int64),
        ("mask_label", vp), ("mask_stride_b", C.c_int64), ("mask_stride_n", C.c_int64), ("mask_dtype", C.c_int32),
        ("thr", C.c_float), ("loss", vp), ("iou_bev", vp), ("iou_3d", vp), ("acc", vp)]


MASK_U8, MASK_F32 = 0, 1


class TrackArgs(C.Structure):
    """dal3_track_args"""
    _fields_ = [("S", C.c_int64), ("F", C.c_int64), ("K", C.c_int64), ("seq_offsets", vp), ("frame_offsets", vp),
                ("ct", vp), ("tracking", vp), ("label", vp), ("score", vp), ("max_dist", C.c_float * 3),
                ("max_age", C.c_int32), ("score_thresh", C.c_double), ("capacity", C.c_int64),
                ("max_workgroups", C.c_int32), ("reserved", C.c_int32), ("id_base", vp), ("box_ids", vp),
                ("tracking_ids", vp), ("out_count", vp), ("id_total", vp), ("status", vp), ("workspace", vp),
                ("workspace_bytes", C.c_size_t)]


class TrackMatchArgs(C.Structure):
    """dal3_track_match_args"""
    _fields_ = [("F", C.c_int64), ("K", C.c_int64), ("frame_offsets", vp), ("out_count", vp), ("box_ids", vp),
                ("tracking_ids", vp), ("id_base", vp), ("boxes", vp), ("gt_offsets", vp), ("gt_boxes", vp),
                ("thr", C.c_float), ("reserved", C.c_int32), ("match_frame", vp), ("match_obj", vp), ("status", vp),
                ("workspace", vp), ("workspace_bytes", C.c_size_t)]


TRACK_MAX_CAPACITY = 65536
TRACK_OVERFLOW, TRACK_BAD_LABEL, TRACK_BAD_ID = 1, 2, 4


class GroupArgs(C.Structure):
    """dal3_group_args"""
    _fields_ = [("E", C.c_int64), ("T", C.c_int64), ("F", C.c_int64), ("keys", vp), ("key_base", vp), ("key_bias", C.c_int64),
                ("frame_offsets", vp), ("out_count", vp), ("group_start", vp), ("entry", vp), ("n_groups", vp), ("status", vp),
                ("max_workgroups", C.c_int64), ("workspace", vp), ("workspace_bytes", C.c_size_t)]


class TrackFeatureArgs(C.Structure):
    """dal3_track_feature_args"""
    _fields_ = [("T", C.c_int64), ("E", C.c_int64), ("group_start", vp), ("entry", vp), ("n_groups", vp), ("center", vp), ("type", vp),
                ("score", vp), ("n_points", vp), ("match", vp), ("n", vp), ("type0", vp), ("match_last", vp),
                ("points_sum", vp), ("best", vp), ("keep", vp), ("feature", vp), ("max_workgroups", C.c_int64)]


class GtTableArgs(C.Structure):
    """dal3_gt_table_args"""
    _fields_ = [("T", C.c_int64), ("E", C.c_int64), ("F", C.c_int64), ("group_start", vp), ("entry", vp), ("box", vp),
                ("frame", vp), ("pose", vp), ("box_global", vp), ("vel", vp), ("n", vp), ("dist", vp), ("max_vel", vp),
                ("is_static", vp), ("status", vp), ("max_workgroups", C.c_int64)]


class MotionClassifyArgs(C.Structure):
    """dal3_motion_classify_args"""
    _fields_ = [("T", C.c_int64), ("feature", vp), ("keep", vp), ("w", C.c_double * 2), ("b", C.c_double), ("decision", vp),
                ("is_static", vp), ("static_ids", vp), ("dynamic_ids", vp), ("counts", vp), ("max_workgroups", C.c_int64),
                ("workspace", vp), ("workspace_bytes", C.c_size_t)]


MOTION_BAD_KEY = 8


class ScoreAcc(C.Structure):
    """dal3_score_acc (72 bytes)"""
    _fields_ = [("sum_iou_bev", C.c_double), ("sum_iou_3d", C.c_double), ("n_iou_3d_pass", C.c_uint64),
                ("n_type", C.c_uint64 * 4), ("n_scored", C.c_uint64), ("n_samples", C.c_uint64)]


class ScoreArgs(C.Structure):
    """dal3_score_args"""
    _fields_ = [("S", C.c_int64), ("R", C.c_int64), ("F", C.c_int64), ("boxes", vp), ("box_row", vp), ("frame", vp),
                ("pose_inv", vp), ("gt", vp), ("has_gt", vp), ("type", vp), ("gt_f64", C.c_int32),
                ("max_workgroups", C.c_int32), ("thr", C.c_float * 3), ("thr_other", C.c_float), ("iou_bev", vp),
                ("iou_3d", vp), ("pred_box", vp), ("label_box", vp), ("acc", vp), ("workspace", vp),
                ("workspace_bytes", C.c_size_t)]


class BestGtArgs(C.Structure):
    """dal3_best_gt_args"""
    _fields_ = [("Q", C.c_int64), ("F", C.c_int64), ("G", C.c_int64), ("queries", vp), ("query_frame", vp),
                ("gt_offsets", vp), ("gt_boxes", vp), ("boxes_f64", C.c_int32), ("max_workgroups", C.c_int32),
                ("best_iou_3d", vp), ("best_iou_bev", vp), ("best_index", vp)]


NMS_MAX_PRE = 65536
NMS_ROTATE, NMS_CIRCLE = 0, 1
NMS_TOO_MANY, NMS_BAD_SEGMENT, DECODE_OVERFLOW = 16, 32, 64


class NmsArgs(C.Structure):
    """dal3_nms_args"""
    _fields_ = [("F", C.c_int64), ("K", C.c_int64), ("seg_offsets", vp), ("seg_offsets_host", vp), ("seg_count", vp),
                ("boxes", vp), ("scores", vp), ("box_stride", C.c_int64), ("yaw_col", C.c_int32), ("boxes_f64", C.c_int32),
                ("mode", C.c_int32), ("thresh", C.c_float), ("pre_max", C.c_int64), ("post_max", C.c_int64),
                ("stride", C.c_int64), ("max_workgroups", C.c_int32), ("mirror", C.c_int32), ("keep", vp),
                ("keep_count", vp), ("order", vp), ("status", vp), ("workspace", vp), ("workspace_bytes", C.c_size_t)]


class Map(C.Structure):
    """dal3_map: a float32 (B, H, W, C) view by element strides"""
    _fields_ = [("data", vp), ("stride_b", C.c_int64), ("stride_h", C.c_int64), ("stride_w", C.c_int64),
                ("stride_c", C.c_int64)]


def nchw_map(t):
    """a logical (B, C, H, W) float32 tensor of any strides -> dal3_map (no copy)"""
    return Map(ptr(t), t.stride(0), t.stride(2), t.stride(3), t.stride(1))


class CenterDecodeArgs(C.Structure):
    """dal3_center_decode_args"""
    _fields_ = [("B", C.c_int64), ("H", C.c_int64), ("W", C.c_int64), ("C", C.c_int32), ("has_range", C.c_int32),
                ("hm", Map), ("reg", Map), ("height", Map), ("dim", Map), ("rot", Map), ("vel", Map),
                ("out_size_factor", C.c_float), ("voxel_size", C.c_float * 2), ("pc_range", C.c_float * 2),
                ("score_threshold", C.c_float), ("range", C.c_float * 6), ("F", C.c_int64), ("K", C.c_int64),
                ("seg_first", C.c_int64), ("seg_step", C.c_int64), ("seg_offsets", vp), ("boxes", vp), ("scores", vp),
                ("labels", vp), ("cell", vp), ("seg_count", vp), ("status", vp), ("max_workgroups", C.c_int64),
                ("workspace", vp), ("workspace_bytes", C.c_size_t)]


class CenterDecodeFlip4Args(C.Structure):
    """dal3_center_decode_flip4_args"""
    _fields_ = [("decode", CenterDecodeArgs)]


SWEEP_MAX = 16


class SweepSegment(C.Structure):
    """dal3_sweep_segment"""
    _fields_ = [("xyz", vp), ("feature", vp), ("n", C.c_int64), ("out_row", C.c_int64), ("matrix", C.c_double * 12),
                ("time", C.c_float), ("has_transform", C.c_int32)]


PILLAR_OVERFLOW = 128
PILLAR_PACK_FLOATS = 5120


class VoxelizeArgs(C.Structure):
    """dal3_voxelize_args"""
    _fields_ = [("B", C.c_int64), ("N", C.c_int64), ("points", vp), ("point_stride", C.c_int64), ("C", C.c_int32),
                ("reverse_index", C.c_int32), ("point_offsets", vp), ("point_offsets_host", vp), ("voxel_size", C.c_float * 3),
                ("pc_range", C.c_float * 6), ("grid", C.c_int32 * 3), ("max_points", C.c_int32), ("max_voxels", C.c_int64),
                ("capacity", C.c_int64), ("voxels", vp), ("coordinates", vp), ("num_points", vp), ("voxel_offsets", vp),
                ("status", vp), ("max_workgroups", C.c_int64), ("workspace", vp), ("workspace_bytes", C.c_size_t)]


class PillarFeatureArgs(C.Structure):
    """dal3_pillar_feature_args"""
    _fields_ = [("P", C.c_int64), ("n_pillars", vp), ("voxels", vp), ("num_points", vp), ("coordinates", vp), ("C", C.c_int32),
                ("max_points", C.c_int32), ("n_layers", C.c_int32), ("c_out", C.c_int32), ("vx", C.c_float), ("vy", C.c_float),
                ("x_offset", C.c_float), ("y_offset", C.c_float), ("packed", vp), ("features", vp), ("canvas", vp),
                ("canvas_B", C.c_int64), ("ny", C.c_int64), ("nx", C.c_int64), ("max_workgroups", C.c_int64)]


PILLAR_TRAIN_SLICE = 128                        # DAL3_PILLAR_TRAIN_SLICE: the pillars of one partial sum of the reader's training step
PILLAR_TRAIN_SAVED_FLOATS = 512
_p2 = vp * 2


class PillarTrainArgs(C.Structure):
    """dal3_pillar_train_args"""
    _fields_ = [("P", C.c_int64), ("n_pillars", vp), ("voxels", vp), ("num_points", vp), ("coordinates", vp), ("C", C.c_int32),
                ("max_points", C.c_int32), ("n_layers", C.c_int32), ("c_out", C.c_int32), ("vx", C.c_float), ("vy", C.c_float),
                ("x_offset", C.c_float), ("y_offset", C.c_float), ("layers", C.POINTER(Layer)), ("eps", C.c_double),
                ("momentum", C.c_double * 2), ("running_mean", _p2), ("running_var", _p2), ("num_batches_tracked", _p2),
                ("saved", vp), ("features", vp), ("canvas", vp), ("canvas_B", C.c_int64), ("ny", C.c_int64), ("nx", C.c_int64),
                ("grad", vp), ("grad_stride", C.c_int64 * 4), ("dW", _p2), ("dgamma", _p2), ("dbeta", _p2),
                ("max_workgroups", C.c_int64), ("workspace", vp), ("workspace_bytes", C.c_size_t)]


CONV2D_3X3, CONV2D_1X1, CONV2D_DECONV2, CONV2D_DECONV4 = range(4)


class Conv2dArgs(C.Structure):
    """dal3_conv2d_args"""
    _fields_ = [("kind", C.c_int32), ("stride", C.c_int32), ("relu", C.c_int32), ("c_in", C.c_int32), ("c_out", C.c_int32),
                ("y_channels", C.c_int32), ("y_channel_offset", C.c_int32), ("max_workgroups", C.c_int32), ("B", C.c_int64),
                ("H", C.c_int64), ("W", C.c_int64), ("x", Map), ("y", Map), ("packed", vp)]


class Conv2dLpArgs(C.Structure):
    """dal3_conv2d_lp_args"""
    _fields_ = [("kind", C.c_int32), ("stride", C.c_int32), ("relu", C.c_int32), ("c_in", C.c_int32), ("c_out", C.c_int32),
                ("y_channels", C.c_int32), ("y_channel_offset", C.c_int32), ("max_workgroups", C.c_int32), ("dtype", C.c_int32),
                ("reserved", C.c_int32), ("B", C.c_int64), ("H", C.c_int64), ("W", C.c_int64), ("x", Map), ("y", Map),
                ("packed", vp)]


CONV2D_WGRAD_SLICE = 4096                       # DAL3_CONV2D_WGRAD_SLICE: the pixels of one partial sum of dal3_conv2d_wgrad


class Conv2dDgradArgs(C.Structure):
    """dal3_conv2d_dgrad_args"""
    _fields_ = [("kind", C.c_int32), ("stride", C.c_int32), ("c_in", C.c_int32), ("c_out", C.c_int32), ("max_workgroups", C.c_int32),
                ("reserved", C.c_int32), ("B", C.c_int64), ("H", C.c_int64), ("W", C.c_int64), ("dy", Map), ("dx", Map), ("packed", vp)]


class Conv2dWgradArgs(C.Structure):
    """dal3_conv2d_wgrad_args"""
    _fields_ = [("kind", C.c_int32), ("stride", C.c_int32), ("c_in", C.c_int32), ("c_out", C.c_int32), ("max_workgroups", C.c_int32),
                ("reserved", C.c_int32), ("B", C.c_int64), ("H", C.c_int64), ("W", C.c_int64), ("x", Map), ("dy", Map), ("dw", vp),
                ("db", vp), ("workspace", vp), ("workspace_bytes", C.c_size_t)]


SP_OVERFLOW, SP_BAD_COORD, SP_DUPLICATE, SP_BAD_WEIGHT = 256, 512, 1024, 2048
_i3 = C.c_int32 * 3


class SpSortArgs(C.Structure):
    """dal3_sp_sort_args"""
    _fields_ = [("B", C.c_int64), ("shape", _i3), ("reserved", C.c_int32), ("capacity", C.c_int64), ("n", vp), ("indices", vp),
                ("sorted_key", vp), ("sorted_pos", vp), ("status", vp), ("max_workgroups", C.c_int64), ("workspace", vp),
                ("workspace_bytes", C.c_size_t)]


class SpDownsampleArgs(C.Structure):
    """dal3_sp_downsample_args"""
    _fields_ = [("B", C.c_int64), ("in_shape", _i3), ("out_shape", _i3), ("kernel", _i3), ("stride", _i3), ("padding", _i3),
                ("reserved", C.c_int32), ("in_capacity", C.c_int64), ("n_in", vp), ("in_indices", vp), ("out_capacity", C.c_int64),
                ("out_indices", vp), ("out_key", vp), ("n_out", vp), ("status", vp), ("max_workgroups", C.c_int64),
                ("workspace", vp), ("workspace_bytes", C.c_size_t)]


class SpTableArgs(C.Structure):
    """dal3_sp_table_args"""
    _fields_ = [("B", C.c_int64), ("in_shape", _i3), ("out_shape", _i3), ("kernel", _i3), ("stride", _i3), ("padding", _i3),
                ("reserved", C.c_int32), ("out_capacity", C.c_int64), ("n_out", vp), ("out_indices", vp), ("in_capacity", C.c_int64),
                ("n_in", vp), ("in_key", vp), ("in_pos", vp), ("table", vp), ("max_workgroups", C.c_int64)]


class SpConvArgs(C.Structure):
    """dal3_sp_conv_args"""
    _fields_ = [("taps", C.c_int32), ("c_in", C.c_int32), ("c_out", C.c_int32), ("relu", C.c_int32), ("center_tap", C.c_int32),
                ("reserved", C.c_int32), ("in_capacity", C.c_int64), ("x", vp), ("out_capacity", C.c_int64), ("n_out", vp),
                ("table", vp), ("packed", vp), ("residual", vp), ("y", vp), ("canvas", vp), ("out_indices", vp),
                ("canvas_B", C.c_int64), ("canvas_shape", _i3), ("reserved2", C.c_int32), ("status", vp),
                ("max_workgroups", C.c_int64)]


class SpConvLpArgs(C.Structure):
    """dal3_sp_conv_lp_args"""
    _fields_ = SpConvArgs._fields_ + [("dtype", C.c_int32), ("x16", vp), ("y16", vp)]


SP_WGRAD_SLICE = 1024                           # DAL3_SP_WGRAD_SLICE: the sites of one partial sum of dal3_sp_wgrad


class SpTableTransposedArgs(C.Structure):
    """dal3_sp_table_transposed_args"""
    _fields_ = [("B", C.c_int64), ("in_shape", _i3), ("out_shape", _i3), ("kernel", _i3), ("stride", _i3), ("padding", _i3),
                ("reserved", C.c_int32), ("in_capacity", C.c_int64), ("n_in", vp), ("in_indices", vp), ("out_capacity", C.c_int64),
                ("n_out", vp), ("out_key", vp), ("table", vp), ("max_workgroups", C.c_int64)]


class SpWgradArgs(C.Structure):
    """dal3_sp_wgrad_args"""
    _fields_ = [("taps", C.c_int32), ("c_in", C.c_int32), ("c_out", C.c_int32), ("reserved", C.c_int32), ("in_capacity", C.c_int64),
                ("x", vp), ("out_capacity", C.c_int64), ("n_out", vp), ("table", vp), ("dy", vp), ("dw", vp), ("db", vp),
                ("max_workgroups", C.c_int64), ("workspace", vp), ("workspace_bytes", C.c_size_t)]


ROI_OVERFLOW = 4096
ROI_MAX_TASKS, ROI_MAX_WIDTH = 16, 256
_f2 = C.c_float * 2


class BevGatherArgs(C.Structure):
    """dal3_bev_gather_args"""
    _fields_ = [("B", C.c_int64), ("H", C.c_int64), ("W", C.c_int64), ("C", C.c_int32), ("sample_index", C.c_int32), ("map", Map),
                ("n", C.c_int64), ("xy", vp), ("xy_stride", C.c_int64), ("sample", vp), ("pc_start", _f2), ("voxel_size", _f2),
                ("out_stride", C.c_float), ("points_per_row", C.c_int32), ("out", vp), ("out_row_stride", C.c_int64),
                ("out_col_offset", C.c_int64)]


class RoiShape(C.Structure):
    """dal3_roi_shape"""
    _fields_ = [("c_in", C.c_int32), ("n_shared", C.c_int32), ("n_cls", C.c_int32), ("n_reg", C.c_int32), ("shared", _i3),
                ("cls", _i3), ("reg", _i3), ("num_class", C.c_int32), ("code_size", C.c_int32)]


class RoiHeadArgs(C.Structure):
    """dal3_roi_head_args"""
    _fields_ = [("shape", RoiShape), ("packed", vp), ("B", C.c_int64), ("M", C.c_int64), ("num_point", C.c_int32), ("C", C.c_int32),
                ("T", C.c_int32), ("box_cols", C.c_int32), ("K", C.c_int64), ("keep_stride", C.c_int64), ("boxes", vp), ("scores", vp),
                ("labels", vp), ("keep", vp), ("keep_count", vp), ("seg_offsets", vp), ("label_base", C.c_int32 * ROI_MAX_TASKS),
                ("bev", Map), ("H", C.c_int64), ("W", C.c_int64), ("pc_start", _f2), ("voxel_size", _f2), ("out_stride", C.c_float),
                ("rois", vp), ("roi_scores", vp), ("roi_features", vp), ("out_boxes", vp), ("out_scores", vp), ("out_labels", vp),
                ("out_counts", vp), ("out_features", vp), ("box_preds", vp), ("cls_preds", vp), ("status", vp), ("workspace", vp),
                ("workspace_bytes", C.c_size_t)]


ROI_NO_SAMPLE = 8192
ROI_CLS_SCORE = {"roi_iou": 0, "cls": 1}
ROI_TRAIN_MAX_M, ROI_TRAIN_MAX_R, ROI_TRAIN_MAX_G = 512, 512, 1024


class RoiTargetsArgs(C.Structure):
    """dal3_roi_targets_args"""
    _fields_ = [("B", C.c_int64), ("M", C.c_int64), ("R", C.c_int64), ("G", C.c_int64), ("code_size", C.c_int32),
                ("reserved0", C.c_int32), ("T", C.c_int32), ("reserved", C.c_int32), ("K", C.c_int64), ("keep_stride", C.c_int64),
                ("boxes", vp), ("scores", vp), ("labels", vp), ("keep", vp), ("keep_count", vp), ("seg_offsets", vp),
                ("label_base", C.c_int32 * ROI_MAX_TASKS), ("rois", vp), ("roi_scores", vp), ("roi_labels", vp), ("gt", vp),
                ("draws", vp), ("fg_per_image", C.c_int32), ("cls_score_type", C.c_int32), ("reg_fg_thresh", C.c_float),
                ("cls_fg_thresh", C.c_float), ("cls_bg_thresh", C.c_float), ("cls_bg_thresh_lo", C.c_float),
                ("cls_thresh_span", C.c_float), ("reserved2", C.c_float), ("hard_bg_ratio", C.c_double), ("slot", vp), ("sample", vp),
                ("out_rois", vp), ("out_labels", vp), ("out_scores", vp), ("gt_iou", vp), ("gt_src", vp), ("reg_valid", vp),
                ("cls_labels", vp), ("gt_of_rois", vp), ("out_boxes", vp), ("status", vp)]


CENTER_OVERFLOW = 16384
CENTER_MAX_OBJS, CENTER_MAX_CLASSES, CENTER_MAX_COLS = 1024, 64, 10
_pT = vp * ROI_MAX_TASKS


class CenterTargetsArgs(C.Structure):
    """dal3_center_targets_args"""
    _fields_ = [("B", C.c_int64), ("G", C.c_int64), ("H", C.c_int64), ("W", C.c_int64), ("T", C.c_int32), ("max_objs", C.c_int32),
                ("num_class", C.c_int32 * ROI_MAX_TASKS), ("gt", vp), ("pc_start", _f2), ("voxel_size", _f2),
                ("out_size_factor", C.c_float), ("min_radius", C.c_int32), ("gaussian_overlap", C.c_double), ("hm", _pT),
                ("anno_box", _pT), ("ind", _pT), ("mask", _pT), ("cat", _pT), ("status", vp)]


class CenterLossArgs(C.Structure):
    """dal3_center_loss_args"""
    _fields_ = [("B", C.c_int64), ("H", C.c_int64), ("W", C.c_int64), ("C", C.c_int32), ("n_cols", C.c_int32), ("max_objs", C.c_int32),
                ("reserved", C.c_int32), ("hm", Map), ("reg", Map), ("height", Map), ("dim", Map), ("rot", Map), ("vel", Map),
                ("target_hm", vp), ("anno_box", vp), ("ind", vp), ("mask", vp), ("cat", vp),
                ("code_weights", C.c_float * CENTER_MAX_COLS), ("weight", C.c_float), ("reserved2", C.c_float), ("out", vp),
                ("grad", vp), ("workspace", vp), ("workspace_bytes", C.c_size_t)]


AUG_TOO_MANY, AUG_OVERFLOW, AUG_BAD_ROW = 32768, 65536, 131072
AUG_MAX_BOXES, AUG_MAX_CAND = 1024, 64


class GtPasteArgs(C.Structure):
    """dal3_gt_paste_args"""
    _fields_ = [("B", C.c_int64), ("max_gt", C.c_int32), ("max_cand", C.c_int32), ("gt_boxes", vp), ("gt_classes", vp),
                ("gt_counts", vp), ("cand_boxes", vp), ("cand_group", vp), ("cand_counts", vp), ("accept", vp), ("coll", vp),
                ("status", vp)]


class AugmentPointsArgs(C.Structure):
    """dal3_augment_points_args"""
    _fields_ = [("B", C.c_int64), ("n", C.c_int64), ("n_scene", C.c_int64), ("db_rows", C.c_int64), ("F", C.c_int32),
                ("transform", C.c_int32), ("max_cand", C.c_int64), ("scene", vp), ("scene_offsets", vp), ("db_points", vp),
                ("out_offsets", vp), ("cand_counts", vp), ("cand_seg_start", vp), ("cand_rows", vp), ("cand_db_row", vp),
                ("cand_boxes", vp), ("accept", vp), ("keys", vp), ("xform", vp), ("out", vp), ("status", vp),
                ("max_workgroups", C.c_int64), ("workspace", vp), ("workspace_bytes", C.c_size_t)]


class AugmentBoxesArgs(C.Structure):
    """dal3_augment_boxes_args"""
    _fields_ = [("B", C.c_int64), ("max_gt", C.c_int32), ("max_cand", C.c_int32), ("max_objs", C.c_int32), ("n_classes", C.c_int32),
                ("transform", C.c_int32), ("reserved", C.c_int32), ("gt_boxes", vp), ("gt_classes", vp), ("gt_counts", vp),
                ("cand_boxes", vp), ("cand_classes", vp), ("cand_counts", vp), ("accept", vp), ("xform", vp),
                ("range", C.c_float * 4), ("out", vp), ("out_count", vp), ("status", vp)]


OPTIM_CHUNK, OPTIM_NORM_SPAN = 4096, 16384      # DAL3_OPTIM_CHUNK, DAL3_OPTIM_NORM_SPAN
OPTIM_TRUE_WD, OPTIM_CLIP, OPTIM_FUSED_ZERO = 1, 2, 4
# dal3_optim_hyper's 8-byte slots, as indices into the block seen as int64 or as float64
(OPTIM_STEP, OPTIM_LR, OPTIM_BETA1, OPTIM_BETA2, OPTIM_EPS, OPTIM_WD, OPTIM_MAX_NORM, OPTIM_FLAGS, OPTIM_TOTAL_STEP,
 OPTIM_TABLE, OPTIM_SLOTS) = range(11)


class OptimChunk(C.Structure):
    """dal3_optim_chunk (24 bytes)"""
    _fields_ = [("param", vp), ("offset", C.c_int64), ("count", C.c_int32), ("decay", C.c_int32)]


# every symbol include/dal3.h declares: (restype, argtypes)
_i, _i64, _u64, _sz = C.c_int, C.c_int64, C.c_uint64, C.c_size_t
SIGNATURES = {
    "dal3_version": (_i, []),
    "dal3_last_error": (C.c_char_p, []),
    "dal3_mean_size": (C.POINTER(C.c_float), []),
    "dal3_pack_weights": (_i, [_i, C.POINTER(Layer), _i, _i, vp, C.POINTER(_sz), vp]),
    "dal3_ins_seg_workspace_bytes": (_sz, [_i]),
    "dal3_ins_seg_plan_layout": (_i, [_i, C.POINTER(_sz), C.POINTER(_i)]),
    "dal3_ins_seg_encoder_route": (_i, [_i, _i, _i]),
    "dal3_ins_seg_decode_route": (_i, [vp, _i, _i, _i]),
    "dal3_ins_seg_forward": (_i, [vp, _i, _i, BCN, _i, _i, vp, vp, vp, vp, _sz, vp]),
    "dal3_ins_seg_encode": (_i, [vp, _i, _i, BCN, _i, _i, vp, vp]),
    "dal3_ins_seg_global_bias": (_i, [vp, _i, vp, _i, vp, vp]),
    "dal3_ins_seg_decode": (_i, [vp, _i, _i, BCN, _i, _i, vp, vp, vp, vp]),
    "dal3_gather_workspace_bytes": (_sz, [_i, _i]),
    "dal3_segment_counts": (_i, [vp, _i, _i, vp, vp]),
    "dal3_mask_compact_sample": (_i, [vp, BCN, _i, _i, _i, _i, _i, vp, _u64, _i64, vp, vp, vp, vp, _sz, vp]),
    "dal3_mask_compact_sample_step": (_i, [vp, BCN, _i, _i, _i, _i, _u64, vp, _i64, vp, vp, vp, vp, _sz, vp]),
    "dal3_point_head_workspace_bytes": (_sz, [_i]),
    "dal3_point_head_forward": (_i, [_i, vp, _i, BCN, _i, _i, vp, _i64, vp, _sz, vp]),
    "dal3_point_head_pool_workspace_bytes": (_sz, [_i, _i]),
    "dal3_point_head_screen_min_tiles": (_i, []),
    "dal3_point_head_route": (_i, [_i, _i, _i, _i]),
    "dal3_point_head_screen_stride": (_i, []),
    "dal3_point_head_pool": (_i, [_i, vp, _i, BCN, _i, _i, vp, vp, vp, _sz, vp]),
    "dal3_dynamic_box_est_forward": (_i, [vp, vp, _i, vp, vp, _sz, vp]),
    "dal3_decode_boxes": (_i, [vp, _i, vp, _i64, _i, vp, _i64, vp, _i64, vp, vp, vp, vp, vp]),
    "dal3_recenter_rotz": (_i, [vp, _i, _i, vp, vp, vp, vp, vp, vp, vp]),
    "dal3_static_crop_prep": (_i, [vp, vp, vp, vp, vp, _i, _i, _u64, _i64, vp, vp, vp]),
    "dal3_dynamic_item_prep": (_i, [vp, vp, vp, vp, vp, vp, vp, vp, _i, _i, _i, _i, _u64, _i64, vp, vp, vp, vp]),
    "dal3_writeback_boxes": (_i, [vp, vp, vp, vp, vp, vp, vp, vp, vp, _i, _i64, vp, vp, vp]),
    "dal3_static_crop_labels": (_i, [vp, vp, vp, vp, _i, _i, _u64, _i64, vp, vp, vp]),
    "dal3_dynamic_item_labels": (_i, [vp, vp, vp, vp, vp, vp, vp, _i, _i, _i, _u64, _i64, vp, vp, vp, vp, vp]),
    "dal3_points_in_boxes": (_i, [vp, _i, _i64, _i64, vp, _i, _i, vp, vp]),
    "dal3_box_iou_pairwise": (_i, [vp, _i64, vp, _i64, _i, vp, vp, vp]),
    "dal3_box_iou_paired": (_i, [vp, vp, _i64, _i, vp, vp, vp]),
    "dal3_box_estimation_metrics": (_i, [C.POINTER(BoxMetricArgs), vp]),
    "dal3_track_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "dal3_track": (_i, [C.POINTER(TrackArgs), vp]),
    "dal3_track_match_workspace_bytes": (_sz, [_i64]),
    "dal3_track_match": (_i, [C.POINTER(TrackMatchArgs), vp]),
    "dal3_group_workspace_bytes": (_sz, [_i64, _i64]),
    "dal3_group_by_key": (_i, [C.POINTER(GroupArgs), vp]),
    "dal3_track_features": (_i, [C.POINTER(TrackFeatureArgs), vp]),
    "dal3_gt_table": (_i, [C.POINTER(GtTableArgs), vp]),
    "dal3_motion_classify_workspace_bytes": (_sz, [_i64]),
    "dal3_motion_classify": (_i, [C.POINTER(MotionClassifyArgs), vp]),
    "dal3_score_workspace_bytes": (_sz, [_i64]),
    "dal3_score_tracks": (_i, [C.POINTER(ScoreArgs), vp]),
    "dal3_best_gt_iou": (_i, [C.POINTER(BestGtArgs), vp]),
    "dal3_nms_workspace_bytes": (_sz, [_i64, _i]),
    "dal3_nms": (_i, [C.POINTER(NmsArgs), vp]),
    "dal3_center_decode_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "dal3_center_decode": (_i, [C.POINTER(CenterDecodeArgs), vp]),
    "dal3_center_decode_flip4_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "dal3_center_decode_flip4": (_i, [C.POINTER(CenterDecodeFlip4Args), vp]),
    "dal3_flip4_points": (_i, [vp, _i64, C.c_int32, vp, _i64, vp, vp, _i64, vp]),
    "dal3_sweep_merge": (_i, [vp, _i64, C.c_int32, _i64, vp, vp, _i64, vp]),
    "dal3_voxelize_workspace_bytes": (_sz, [_i64, _i64]),
    "dal3_voxelize": (_i, [C.POINTER(VoxelizeArgs), vp]),
    "dal3_pillar_pack": (_i, [C.POINTER(Layer), _i, _i, C.c_double, vp, vp]),
    "dal3_pillar_features": (_i, [C.POINTER(PillarFeatureArgs), vp]),
    "dal3_pillar_train_workspace_bytes": (_sz, [_i64, _i]),
    "dal3_pillar_train_forward": (_i, [C.POINTER(PillarTrainArgs), vp]),
    "dal3_pillar_train_backward": (_i, [C.POINTER(PillarTrainArgs), vp]),
    "dal3_pillar_scatter": (_i, [vp, vp, _i64, vp, _i, vp, _i64, _i64, _i64, vp]),
    "dal3_voxel_mean": (_i, [vp, vp, _i64, vp, _i, _i, vp, vp]),
    "dal3_conv2d_pack_floats": (_sz, [_i, _i, _i]),
    "dal3_conv2d_pack": (_i, [C.POINTER(Layer), _i, C.c_double, vp, vp]),
    "dal3_conv2d": (_i, [C.POINTER(Conv2dArgs), vp]),
    "dal3_conv2d_lp_pack_bytes": (_sz, [_i, _i, _i]),
    "dal3_conv2d_lp_pack": (_i, [C.POINTER(Layer), _i, C.c_double, _i, vp, vp]),
    "dal3_conv2d_lp": (_i, [C.POINTER(Conv2dLpArgs), vp]),
    "dal3_conv2d_dgrad_pack_floats": (_sz, [_i, _i, _i]),
    "dal3_conv2d_dgrad_pack": (_i, [vp, _i, _i, _i, vp, vp]),
    "dal3_conv2d_dgrad": (_i, [C.POINTER(Conv2dDgradArgs), vp]),
    "dal3_conv2d_wgrad_workspace_bytes": (_sz, [_i, _i, _i, _i, _i64, _i64, _i64]),
    "dal3_conv2d_wgrad": (_i, [C.POINTER(Conv2dWgradArgs), vp]),
    "dal3_sp_sort_workspace_bytes": (_sz, [_i64]),
    "dal3_sp_sort": (_i, [C.POINTER(SpSortArgs), vp]),
    "dal3_sp_downsample_workspace_bytes": (_sz, [_i64, _i]),
    "dal3_sp_downsample": (_i, [C.POINTER(SpDownsampleArgs), vp]),
    "dal3_sp_table": (_i, [C.POINTER(SpTableArgs), vp]),
    "dal3_sp_conv_pack_floats": (_sz, [_i, _i, _i]),
    "dal3_sp_conv_pack": (_i, [C.POINTER(Layer), _i, C.c_double, vp, vp, vp]),
    "dal3_sp_conv": (_i, [C.POINTER(SpConvArgs), vp]),
    "dal3_sp_conv_lp_pack_bytes": (_sz, [_i, _i, _i]),
    "dal3_sp_conv_lp_pack": (_i, [C.POINTER(Layer), _i, C.c_double, _i, vp, vp, vp]),
    "dal3_sp_conv_lp": (_i, [C.POINTER(SpConvLpArgs), vp]),
    "dal3_sp_table_transposed": (_i, [C.POINTER(SpTableTransposedArgs), vp]),
    "dal3_sp_wgrad_workspace_bytes": (_sz, [_i, _i, _i, _i64]),
    "dal3_sp_wgrad": (_i, [C.POINTER(SpWgradArgs), vp]),
    "dal3_bev_gather": (_i, [C.POINTER(BevGatherArgs), vp]),
    "dal3_box_points": (_i, [vp, _i64, _i, _i, vp, vp]),
    "dal3_roi_pack_floats": (_sz, [C.POINTER(RoiShape)]),
    "dal3_roi_pack": (_i, [C.POINTER(RoiShape), C.POINTER(Layer), _i, C.POINTER(C.c_double), vp, vp]),
    "dal3_roi_head_workspace_bytes": (_sz, [_i64, _i64, _i, _i, _i]),
    "dal3_roi_head": (_i, [C.POINTER(RoiHeadArgs), vp]),
    "dal3_roi_post": (_i, [vp, vp, vp, _i64, _i, vp, vp, vp]),
    "dal3_roi_targets": (_i, [C.POINTER(RoiTargetsArgs), vp]),
    "dal3_roi_loss": (_i, [vp, vp, _i64, _i, vp, vp, vp, C.POINTER(C.c_float), C.c_float, C.c_float, vp, vp, vp, vp]),
    "dal3_center_targets": (_i, [C.POINTER(CenterTargetsArgs), vp]),
    "dal3_center_loss_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "dal3_center_loss": (_i, [C.POINTER(CenterLossArgs), vp]),
    "dal3_gt_paste_select": (_i, [C.POINTER(GtPasteArgs), vp]),
    "dal3_augment_points_workspace_bytes": (_sz, [_i64, _i64]),
    "dal3_augment_points": (_i, [C.POINTER(AugmentPointsArgs), vp]),
    "dal3_augment_boxes": (_i, [C.POINTER(AugmentBoxesArgs), vp]),
    "dal3_optim_partials": (_i64, [_i64]),
    "dal3_optim_grad_norm": (_i, [vp, _i64, vp, vp, vp]),
    "dal3_optim_step": (_i, [vp, _i64, vp, vp, vp, _i64, vp, vp, vp]),
    "dal3_optim_total_norm": (_i, [vp, _i64, vp, vp]),
    "dal3_crop_workspace_bytes": (_sz, [_i64, _i64]),
    "dal3_crop_count": (_i, [vp, vp, vp, vp, vp, _i, _i64, _i64, vp, vp, _sz, vp]),
    "dal3_crop_fill": (_i, [vp, vp, vp, vp, vp, _i, _i64, _i64, vp, vp, vp, vp, vp, _i64, vp, _sz, vp]),
    "dal3_crop_starts": (_i, [vp, vp, _i64, vp, vp, vp]),
    "dal3_crop_starts_capped": (_i, [vp, vp, _i64, vp, vp, _i64, vp]),
    "dal3_tr_linear": (_i, [vp, _i64, _i, _i64, vp, vp, _i, vp, _i64, _i, vp, _i64, _i, vp, _i64, _i, vp, _sz, vp]),
    "dal3_tr_linear_workspace_bytes": (_sz, [_i, _i]),
    "dal3_tr_linear_pack_layout": (_i, [_i64, _i, _i64, _i, _i, _i]),
    "dal3_tr_pack_many": (_i, [vp, _i, vp]),
    "dal3_tr_linear_prepacked": (_i, [vp, _i64, _i, _i64, vp, vp, _i, vp, _i64, _i, vp, _i64, _i, vp, _i64, _i, vp, vp]),
    "dal3_tr_linear_x3_layout": (_i, [_i64, _i, _i64, _i, _i, _i]),
    "dal3_tr_linear_x3": (_i, [vp, _i64, _i, _i64, vp, vp, _i, vp, _i64, _i, vp, _i64, vp, vp, vp]),
    "dal3_tr_bnbwd_apply_amax": (_i, [vp, _i64, _i, _i64, vp, _i64, vp, vp, _i64, vp, vp, vp, vp, vp, vp, vp, vp, _i64, vp, vp]),
    "dal3_tr_colred_workspace_bytes": (_sz, [_i64, _i]),
    "dal3_tr_act_colsum": (_i, [vp, _i64, _i, _i64, vp, vp, _i, vp, _i64, vp, _sz, vp, vp]),
    "dal3_tr_colred": (_i, [vp, _i64, _i, _i64, _i, vp, _i64, vp, vp, _i64, vp, vp, vp, vp, vp, _sz, vp, vp]),
    "dal3_tr_pool_coef": (_i, [vp, vp, vp, vp, vp, vp, _i, _i, _i64, vp, vp, vp]),
    "dal3_tr_head2_forward": (_i, [vp, _i64, _i, _i64, vp, vp, _i, vp, _i64, _u64, vp, C.c_float, vp, _i64, vp, vp, vp]),
    "dal3_tr_head2_dgrad": (_i, [vp, _i64, _i, vp, _i64, _u64, vp, C.c_float, vp, _i64, vp, _i64, vp]),
    "dal3_tr_head2_dgrad_bnbwd": (_i, [vp, _i64, _i, vp, _i64, _u64, vp, C.c_float, vp, _i64, vp, _i64, vp, _i64, vp, vp, vp, vp, vp,
                                       vp, vp, vp, vp, vp, vp, _sz, vp]),
    "dal3_tr_head2_wgrad_workspace_bytes": (_sz, [_i64]),
    "dal3_tr_head2_wgrad": (_i, [vp, vp, _i64, _i, _i64, vp, vp, _i, vp, _i64, _u64, vp, C.c_float, vp, _sz, vp, vp]),
    "dal3_tr_conv1_workspace_bytes": (_sz, [_i64, _i]),
    "dal3_tr_conv1_bn_stats": (_i, [vp, _i64, _i64, _i, _i64, vp, _i64, vp, _i, vp, _i64, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp,
                                    vp, vp, vp, _sz, vp]),
    "dal3_tr_conv1_wgrad": (_i, [vp, _i64, vp, _i64, _i, _i64, _i, vp, _sz, vp, vp]),
    "dal3_tr_gather_at": (_i, [vp, _i64, vp, _i64, _i, _i, vp, vp]),
    "dal3_tr_pool_zarg": (_i, [vp, vp, _i64, vp, _i64, vp, _i, _i, _i, _i, vp, vp]),
    "dal3_tr_pool_moments": (_i, [vp, _i64, vp, vp, vp, _i64, _i, _i, vp, vp]),
    "dal3_tr_pool_gv_workspace_bytes": (_sz, [_i]),
    "dal3_tr_pool_gv": (_i, [vp, vp, _i64, vp, _i, _i, vp, vp, vp, _sz, vp]),
    "dal3_tr_pool_dw": (_i, [vp, vp, _i64, vp, vp, vp, _i64, _i, vp, _i, _i, vp, vp]),
    "dal3_tr_pool_sparse": (_i, [vp, vp, vp, _i64, vp, _i64, _i, _i, _i, _i, vp, _i64, vp, vp]),
    "dal3_tr_box_loss": (_i, [vp] * 10 + [_i] + [vp] * 7),
    "dal3_tr_seg_ce_workspace_bytes": (_sz, [_i64]),
    "dal3_tr_seg_ce": (_i, [vp, vp, _i, _i64, vp, vp, vp, _sz, vp]),
    "dal3_tr_linear_red_workspace_bytes": (_sz, [_i64, _i]),
    "dal3_tr_linear_bn_stats": (_i, [vp, _i64, _i, _i64, vp, vp, _i, vp, _i64, vp, _i64, _i, vp, _i64, vp, _i64, vp, vp, vp, vp,
                                     C.c_float, C.c_float, vp, vp, vp, vp, vp, _sz, vp]),
    "dal3_tr_linear_bnbwd_sums": (_i, [vp, _i64, _i, _i64, vp, _i64, _i, vp, _i64, vp, _i64, vp, _i64, vp, vp, vp, vp, vp,
                                       vp, vp, vp, vp, vp, vp, _sz, vp]),
    "dal3_tr_bn_stats": (_i, [vp, _i64, _i, _i64, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp, _sz, vp]),
    "dal3_tr_bnbwd_sums": (_i, [vp, _i64, _i, _i64, vp, _i64, vp, vp, _i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, _sz,
                                vp]),
    "dal3_tr_bn_finalize": (_i, [vp, _i, _i64, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp]),
    "dal3_tr_bnbwd_coef": (_i, [vp, _i, _i64, vp, vp, vp, vp, vp, vp, vp, vp]),
    "dal3_parse_box_pred": (_i, [vp, _i64, _i64, vp, vp, vp, vp, vp, vp, vp, vp]),
    "dal3_parse_box_pred_backward": (_i, [vp, vp, vp, vp, vp, vp, vp, _i64, vp, vp]),
    "dal3_tr_fc_max_rows": (_i, []),
    "dal3_tr_fc_max_act_cin": (_i, []),
    "dal3_tr_fc_forward": (_i, [vp, _i64, _i, _i64, vp, vp, _i, vp, _i64, _i, vp, _i, vp, _i64, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp]),
    "dal3_tr_fc_backward_w": (_i, [vp, _i64, _i64, _i, vp, _i64, vp, vp, vp, vp, vp, vp, vp, vp, _i, _i64, vp, vp, _i, vp, _i64, vp, _i64,
                                   vp, vp]),
    "dal3_tr_bnbwd_apply": (_i, [vp, _i64, _i, _i64, vp, _i64, vp, vp, _i64, vp, vp, vp, vp, vp, vp, vp, vp, _i64, vp]),
    "dal3_tr_bnbwd_apply_segsum_workspace_bytes": (_sz, [_i64, _i]),
    "dal3_tr_bnbwd_apply_segsum": (_i, [vp, _i64, _i, _i64, vp, _i64, vp, vp, vp, vp, vp, vp, vp, vp, _i64, _i64, vp, vp, _sz, vp]),
    "dal3_tr_wgrad_workspace_bytes": (_sz, [_i64, _i, _i]),
    "dal3_tr_wgrad": (_i, [vp, _i64, vp, _i64, vp, vp, _i, _i64, _i, _i, vp, _sz, vp, vp]),
    "dal3_tr_wgrad_final_many": (_i, [C.POINTER(WgradPart), _i, vp]),
    "dal3_tr_wgrad_x3_workspace_bytes": (_sz, [_i64, _i, _i]),
    "dal3_tr_wgrad_x3": (_i, [vp, _i64, vp, _i64, vp, vp, _i, vp, _i64, _i, _i, vp, _sz, vp, vp]),
    "dal3_tr_segmax": (_i, [vp, _i64, _i64, _i, vp, vp, vp, vp, _i64, vp, _sz, vp]),
    "dal3_tr_act_dropout": (_i, [vp, _i64, _i, _i64, vp, vp, _i, vp, _i64, _u64, vp, C.c_float, vp, _i64, vp]),
    "dal3_tr_linear_pool_workspace_bytes": (_sz, [_i, _i, _i64]),
    "dal3_tr_linear_pool": (_i, [vp, _i64, _i, _i64, vp, vp, _i, vp, _i64, vp, vp, vp, _i64, _i, vp, vp, vp, _sz, vp]),
    "dal3_tr_linear_pool_x3": (_i, [vp, _i64, _i, _i64, vp, vp, _i, vp, _i64, vp, vp, vp, _i64, _i, vp, vp, vp, _sz, vp]),
    "dal3_tr_linear_pool_x3_ok": (_i, [_i64, _i, _i64, _i]),
    "dal3_tr_segsum": (_i, [vp, _i64, _i64, _i, vp, _i64, vp]),
    "dal3_maxpool_n": (_i, [vp, _i64, _i64, vp, vp]),
    "dal3_maxpool_n_dtype": (_i, [vp, _i, _i64, _i64, vp, vp]),
    "dal3_shared_mlp_layer": (_i, [C.POINTER(Layer), _i, BCN, _i, _i, vp, vp, _sz, vp]),
    "dal3_shared_mlp_layer_workspace_bytes": (_sz, [_i, _i]),
    "dal3_static_workspace_bytes": (_sz, [_i, _i, _i]),
    "dal3_static_forward": (_i, [C.POINTER(StaticArgs), _i, vp]),
    "dal3_dynamic_workspace_bytes": (_sz, [_i, _i, _i]),
    "dal3_dynamic_forward": (_i, [C.POINTER(DynamicArgs), _i, vp]),
}

_lib = None


def lib():
    """The loaded library; raises (loudly) if it was never built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP library first "
                "(`make -C 3dal_pytorch_amd/csrc` or __graft_entry__.build()). "
                "There is no CPU/eager fallback for the eval-mode forward.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        from . import arch
        lib_mean = [handle.dal3_mean_size()[i] for i in range(9)]
        want = [C.c_float(v).value for row in arch.MEAN_SIZE for v in row]
        if lib_mean != want:                                # two copies of one table: they may not drift apart
            raise RuntimeError(f"lib3dal_hip.so was built with MEAN_SIZE {lib_mean}, arch.MEAN_SIZE is {want}: rebuild the library")
        _lib = handle
    return _lib


def check(rc):
    if rc != OK:
        raise RuntimeError(f"lib3dal_hip error {rc}: {lib().dal3_last_error().decode()}")


def stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return vp(t.data_ptr()) if t is not None else vp(None)


def require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(
            f"{what} lives on {t.device}: the eval-mode forward runs only on an MI355X through "
            "lib3dal_hip.so (no CPU fallback). Move the model and its inputs to the GPU.")


def workspace(nbytes, device):
    """a run kernel's workspace of `nbytes` bytes on `device`; never empty: 8 bytes cover the 8-byte alignment checks of
    dal3_api.hip"""
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)


def host_offsets(offsets, n, name, sized_by, count):
    """the HOST offsets `name` of a run (a list, an array or a CPU tensor; `count` + 1 of them) checked against [0, n]
    -> contiguous int64 array. `sized_by`: what the message says the host needs them for."""
    if torch.is_tensor(offsets):
        if offsets.is_cuda:
            raise TypeError(f"{name} must be on the host (a list, an array or a CPU tensor): {sized_by} from it, and "
                            "reading a device tensor back would be the synchronisation this call avoids")
        offsets = offsets.numpy()
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    if off.size < 1:
        raise ValueError(f"{name} needs {count} + 1 entries")
    if off[0] < 0 or off[-1] > n or np.any(np.diff(off) < 0):
        raise ValueError(f"{name} must be non-decreasing within [0, {n}]")
    return off


STORAGE = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
BCN_NO_SMALL_JOB_KERNELS, BCN_NO_WORKLIST, BCN_NO_LDS_SAMPLER = 1, 2, 4
BCN_NO_DEC_PLAN = 16
BCN_NO_ENC_RESIDENT = 32
BCN_NO_HEAD_RESIDENT = 64
BCN_NO_DEC_PAIR = 128
ENC_ROUTE_LATENCY, ENC_ROUTE_DENSE, ENC_ROUTE_TWO_LAUNCH, ENC_ROUTE_RESIDENT = 0, 1, 2, 3      # dal3_ins_seg_encoder_route
DEC_ROUTE_LATENCY, DEC_ROUTE_ONE_WAVE, DEC_ROUTE_PAIR = 0, 1, 2      # dal3_ins_seg_decode_route
HEAD_ROUTE_LATENCY, HEAD_ROUTE_PER_TILE, HEAD_ROUTE_PERSISTENT, HEAD_ROUTE_TWO_LAUNCH, HEAD_ROUTE_RESIDENT = 0, 1, 2, 3, 4      # dal3_point_head_route
# dal3_bcn.flags of every view bcn() builds (include/dal3.h, DAL3_BCN_*). 0 in normal use; A/B measurements and the
# tests that pin "both kernel families give the same bits" set it around a call (binding-side, the library has no switch).
DISPATCH_FLAGS = 0


def bcn(t):
    """logical (B,C,N) tensor (fp32, or bf16 / fp16 storage read in place) with arbitrary element strides -> dal3_bcn
    (no copy)."""
    assert t.dim() == 3 and t.dtype in STORAGE
    sb, sc, sn = t.stride()
    return BCN(ptr(t), sb, sc, sn, STORAGE[t.dtype], DISPATCH_FLAGS)


def layer_struct(conv, bn):
    """a convolution or nn.Linear (+ optional BatchNorm) -> dal3_layer of raw device pointers. The widths are the
    module's in_channels / out_channels where it has them (a transposed or sparse convolution's weight is not
    (c_out, c_in, ...)), the weight's first two extents otherwise."""
    w = conv.weight
    c_in, c_out = getattr(conv, "in_channels", w.shape[1]), getattr(conv, "out_channels", w.shape[0])
    if not w.is_contiguous() or w.dtype != torch.float32:
        raise RuntimeError("weights must be contiguous fp32")
    L = Layer(ptr(w), ptr(conv.bias), None, None, None, None, c_in, c_out)
    if bn is not None:
        L.bn_weight, L.bn_bias = ptr(bn.weight), ptr(bn.bias)
        L.bn_mean, L.bn_var = ptr(bn.running_mean), ptr(bn.running_var)
    return L


def fold_layer_struct(conv, bn, what="the layer's parameters"):
    """layer_struct for the packers that fold a BatchNorm on the device: every tensor of the (conv, bn) pair, the
    running statistics too, must be on the GPU and contiguous fp32."""
    ts = [conv.weight] + ([conv.bias] if conv.bias is not None else [])
    if bn is not None:
        ts += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
    for t in ts:
        require_gpu(t, what)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("weights must be contiguous fp32")
    return layer_struct(conv, bn)


F16_MAX = 65504.0


def check_f16x3_range(pairs):
    """DAL3_F16X3 (include/dal3.h): a folded weight beyond fp16's largest finite value cannot be split into two halves.
    The shared-MLP kernels are built without NaN semantics (a NaN weight is not guaranteed to reach the outputs), so the
    range is checked HERE, once per packing (one device->host sync per weight change, not per forward), and refused."""
    with torch.no_grad():
        worst = None
        for conv, bn in pairs:
            w = conv.weight.detach().reshape(conv.weight.shape[0], -1).abs().amax(1)
            if bn is not None:
                w = w * (bn.weight.detach() / torch.sqrt(bn.running_var.detach() + 1e-5)).abs()
            m = w.max()
            worst = m if worst is None else torch.maximum(worst, m)
        if worst is not None and not float(worst) < F16_MAX:
            raise ValueError(f"precision 'f16x3': a folded weight of magnitude {float(worst):.3g} is beyond fp16's range "
                             f"({F16_MAX:g}); this head cannot run on the f16x3 kernels (use precision 'fp32')")


def pack(head_kind, pairs, device, dtype=F32):
    """pairs: [(conv_or_linear, bn_or_None), ...] in forward order -> packed uint8 device tensor."""
    if dtype == F16X3:
        check_f16x3_range(pairs)
    arr = (Layer * len(pairs))(*[layer_struct(c, b) for c, b in pairs])
    need = _sz(0)
    check(lib().dal3_pack_weights(head_kind, arr, len(pairs), dtype, None, C.byref(need), None))
    buf = torch.empty(need.value, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 256 == 0
    check(lib().dal3_pack_weights(head_kind, arr, len(pairs), dtype, ptr(buf), C.byref(need), stream()))
    return buf
