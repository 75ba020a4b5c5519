"""CenterPoint's second stage, eval mode, float32, on the GPU through lib3dal_hip.so (dal3_bev_gather, dal3_box_points,
dal3_roi_pack, dal3_roi_head, dal3_roi_post; include/dal3.h holds the definition), under the reference's names, constructor
signatures and checkpoint keys: `BEVFeatureExtractor` (det3d/models/second_stage/bird_eye_view.py), `RoIHead`
(det3d/models/roi_heads/roi_head.py, roi_head_template.py) and `TwoStageDetector` (det3d/models/detectors/two_stage.py),
built from the `model` dict of a config such as
configs/waymo/voxelnet/two_stage/waymo_centerpoint_voxelnet_two_sweep_two_stage_bev_5point_ft_6epoch_freeze_with_vel.py.

`TwoStageDetector` runs its first stage through `single_det.extract_feat`, `single_det.bbox_head` and a `CenterHeadPost`
of its own, whose `decode_nms` leaves the kept rows on the device; `refine` takes them and the neck's NCHW map through the
fused dal3_roi_head (slot resolution, box points, BEV gather, MLP, box prediction, post-processing) with no host round
trip, and `forward` / `detect` read the counts and the status back once, at the end. The modules one by one —
`get_box_center`, `BEVFeatureExtractor`, `reorder_first_stage_pred_and_feature`, `RoIHead`, `post_process` — run the same
device code and give the same bits.

The second stage's training on a frozen first stage (`freeze=True`, the pipeline's ..._ft_6epoch_freeze configs) runs beside
it: `ProposalTargetLayer` and `RoIHead.assign_targets` on dal3_roi_targets (sampling and target encoding for all samples in
one launch, the randomness an input: `draws`), `RoIHead.train_forward` (the three Sequential stacks in train mode on
train.py's Linear + BatchNorm1d + ReLU kernels, Dropout a stock torch op), `get_loss` and its two layer losses on
dal3_roi_loss, `TwoStageDetector.roi_loss` (the device part, nothing read back) and `second_stage_loss`. The first stage's
own loss and training, double-flip, the `voxel_feature` stream and num_class > 1 are not built; each is refused by name.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _hip, pillars, rpn
from .detect import CenterHeadPost, _get, _map, _map_struct


def _f32(t, what, dim):
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor")
    _hip.require_gpu(t, what)
    if t.dtype != torch.float32 or t.dim() != dim:
        raise ValueError(f"{what} must be a {dim}-D float32 tensor, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def box_points(boxes, num_point):
    """TwoStageDetector.get_box_center for one sample: boxes (n, 7 or 9), the rotation in the last column -> (num_point * n,
    3): the centres, then the front, back, left and right mid-edges (dal3_box_points)"""
    boxes = _f32(boxes, "boxes", 2)
    n, cols = boxes.shape
    out = torch.empty((num_point * n, 3), dtype=torch.float32, device=boxes.device)
    _hip.check(_hip.lib().dal3_box_points(_hip.ptr(boxes), n, cols, int(num_point), _hip.ptr(out), _hip.stream()))
    return out


class BEVFeatureExtractor(nn.Module):
    """bird_eye_view.py: bilinear BEV features at the points of each box. forward(example, batch_centers, num_point):
    example['bev_feature'] (B, H, W, C), a permuted view of the neck's NCHW map is fine (no copy is made);
    batch_centers[b] (num_point * n_b, 3), the points' sections one after another -> [(n_b, num_point * C)], section p in
    columns [p * C, (p + 1) * C)."""

    def __init__(self, pc_start, voxel_size, out_stride):
        super().__init__()
        self.pc_start, self.voxel_size, self.out_stride = pc_start, voxel_size, out_stride

    def absl_to_relative(self, absolute):
        a1 = (absolute[..., 0] - self.pc_start[0]) / self.voxel_size[0] / self.out_stride
        a2 = (absolute[..., 1] - self.pc_start[1]) / self.voxel_size[1] / self.out_stride
        return a1, a2

    def _args(self, bev):
        _, H, W, Cn = bev.shape
        a = _hip.BevGatherArgs(B=bev.shape[0], H=H, W=W, C=Cn, map=_map_struct(bev), out_stride=float(self.out_stride))
        a.pc_start[:] = [float(v) for v in self.pc_start[:2]]
        a.voxel_size[:] = [float(v) for v in self.voxel_size[:2]]
        return a

    def forward(self, example, batch_centers, num_point):
        bev = _map(example["bev_feature"], "NHWC", None, "example['bev_feature']")
        B, Cn = bev.shape[0], bev.shape[3]
        if len(batch_centers) != B:
            raise ValueError(f"{len(batch_centers)} lists of centres for {B} samples")
        lib, ret = _hip.lib(), []
        for b in range(B):
            pts = _f32(batch_centers[b], f"batch_centers[{b}]", 2)
            if pts.shape[0] % num_point:
                raise ValueError(f"batch_centers[{b}] holds {pts.shape[0]} points, no multiple of num_point = {num_point}")
            n = pts.shape[0] // num_point
            out = torch.empty((n, num_point * Cn), dtype=torch.float32, device=bev.device)
            for p in range(num_point if n else 0):
                a = self._args(bev)
                sec = pts[p * n:(p + 1) * n]
                a.n, a.xy, a.xy_stride, a.sample, a.sample_index = n, _hip.ptr(sec), pts.stride(0), None, b
                a.points_per_row, a.out, a.out_row_stride, a.out_col_offset = 1, _hip.ptr(out), num_point * Cn, p * Cn
                _hip.check(lib.dal3_bev_gather(a, _hip.stream()))
            ret.append(out)
        return ret

def roi_targets(cfg, code_size, gt_boxes_and_cls, draws=None, *, rois=None, roi_scores=None, roi_labels=None, fused=None, M=None,
                generator=None):
    """dal3_roi_targets. cfg: TARGET_CONFIG. Direct form: rois (B, M, code_size), roi_scores (B, M), roi_labels (B, M); fused
    form: fused = (decode_nms's dict, label_base list) with M slots. gt_boxes_and_cls (B, G, code_size + 1); draws (B, M + R)
    float32 in [0, 1), None: torch.rand with `generator`. Enqueued, nothing read back -> a dict of device tensors: slot,
    sample, rois, boxes (the rois with the rotation back in the last column, dal3_box_points' layout),
    roi_labels (int64), roi_scores, gt_iou_of_rois, gt_of_rois_src, reg_valid_mask (int64), rcnn_cls_labels (float32 for
    roi_iou, int64 for cls), gt_of_rois (encoded), status (1) int32, reg_valid_i32 / cls_labels_f32 (the kernel's own)."""
    R = int(_get(cfg, "ROI_PER_IMAGE"))
    kind = _get(cfg, "CLS_SCORE_TYPE")
    if kind not in _hip.ROI_CLS_SCORE:
        raise NotImplementedError(f"CLS_SCORE_TYPE = {kind!r} (known: {sorted(_hip.ROI_CLS_SCORE)})")
    if not _get(cfg, "SAMPLE_ROI_BY_EACH_CLASS", False):
        raise NotImplementedError("SAMPLE_ROI_BY_EACH_CLASS = False: the class-agnostic assignment is not built")
    slots = M if fused is not None else (rois.shape[1] if torch.is_tensor(rois) and rois.dim() == 3 else 0)
    rows = gt_boxes_and_cls.shape[1] if torch.is_tensor(gt_boxes_and_cls) and gt_boxes_and_cls.dim() == 3 else 0
    if slots > _hip.ROI_TRAIN_MAX_M or R > _hip.ROI_TRAIN_MAX_R or rows > _hip.ROI_TRAIN_MAX_G or R < 1:
        raise ValueError(f"{slots} slots / ROI_PER_IMAGE = {R} / {rows} GT rows: dal3_roi_targets serves up to {_hip.ROI_TRAIN_MAX_M} / "
                         f"{_hip.ROI_TRAIN_MAX_R} / {_hip.ROI_TRAIN_MAX_G}")
    gt = _f32(gt_boxes_and_cls, "gt_boxes_and_cls", 3)
    B, G, cols = gt.shape
    dev = gt.device
    if fused is None:
        rois = _f32(rois, "rois", 3)
        M = rois.shape[1]
        scores = _f32(roi_scores, "roi_scores", 2)
        if not torch.is_tensor(roi_labels) or tuple(roi_labels.shape) != (B, M) or tuple(scores.shape) != (B, M) or rois.shape[0] != B:
            raise ValueError(f"rois {tuple(rois.shape)}, roi_scores {tuple(scores.shape)}, roi_labels and gt_boxes_and_cls {tuple(gt.shape)} "
                             "do not agree on (B, M)")
        if rois.shape[2] != code_size:
            raise ValueError(f"rois have {rois.shape[2]} columns, code_size is {code_size}")
        labels = roi_labels.to(torch.int32).contiguous()
    if cols != code_size + 1:
        raise ValueError(f"gt_boxes_and_cls has {cols} columns, code_size + 1 = {code_size + 1} are needed (the class last)")
    if G == 0:                                  # the reference's single zero row
        gt, G = gt.new_zeros((B, 1, cols)), 1
    if M < 1:
        raise ValueError("no slots")
    if draws is None:
        draws = torch.rand((B, M + R), device=dev, generator=generator)
    draws = _f32(draws, "draws", 2)
    if tuple(draws.shape) != (B, M + R):
        raise ValueError(f"draws must be (B, M + ROI_PER_IMAGE) = ({B}, {M + R}), got {tuple(draws.shape)}")
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(slot=torch.empty((B, R), **i32), sample=torch.empty((B, R), **i32), rois=torch.empty((B, R, code_size), **f32),
               roi_labels=torch.empty((B, R), **i32), roi_scores=torch.empty((B, R), **f32), gt_iou_of_rois=torch.empty((B, R), **f32),
               gt_of_rois_src=torch.empty((B, R, cols), **f32), reg_valid_i32=torch.empty((B, R), **i32),
               cls_labels_f32=torch.empty((B, R), **f32), gt_of_rois=torch.empty((B, R, cols), **f32),
               boxes=torch.empty((B, R, code_size), **f32))
    fg_t, bg_t = float(_get(cfg, "CLS_FG_THRESH")), float(_get(cfg, "CLS_BG_THRESH"))
    a = _hip.RoiTargetsArgs(B=B, M=M, R=R, G=G, code_size=code_size, gt=_hip.ptr(gt), draws=_hip.ptr(draws),
                            fg_per_image=int(np.round(float(_get(cfg, "FG_RATIO")) * R)), cls_score_type=_hip.ROI_CLS_SCORE[kind],
                            reg_fg_thresh=float(_get(cfg, "REG_FG_THRESH")), cls_fg_thresh=fg_t, cls_bg_thresh=bg_t,
                            cls_bg_thresh_lo=float(_get(cfg, "CLS_BG_THRESH_LO")), cls_thresh_span=fg_t - bg_t,
                            hard_bg_ratio=float(_get(cfg, "HARD_BG_RATIO")), slot=_hip.ptr(out["slot"]), sample=_hip.ptr(out["sample"]),
                            out_rois=_hip.ptr(out["rois"]), out_labels=_hip.ptr(out["roi_labels"]), out_scores=_hip.ptr(out["roi_scores"]),
                            gt_iou=_hip.ptr(out["gt_iou_of_rois"]), gt_src=_hip.ptr(out["gt_of_rois_src"]),
                            reg_valid=_hip.ptr(out["reg_valid_i32"]), cls_labels=_hip.ptr(out["cls_labels_f32"]),
                            gt_of_rois=_hip.ptr(out["gt_of_rois"]), out_boxes=_hip.ptr(out["boxes"]))
    if fused is None:
        a.rois, a.roi_scores, a.roi_labels = _hip.ptr(rois), _hip.ptr(scores), _hip.ptr(labels)
        status = torch.zeros(1, **i32)
    else:
        r, label_base = fused
        T = len(label_base)
        if r["B"] != B or r["keep"].shape[0] != T * B or r["boxes"].shape[1] != code_size:
            raise ValueError(f"the first stage's result holds {r['B']} samples in {r['keep'].shape[0]} segments of {r['boxes'].shape[1]} "
                             f"columns; the GT holds {B} samples, code_size is {code_size}")
        if not (r["keep"].is_contiguous() and r["boxes"].is_contiguous() and r["keep"].dtype == torch.int32):
            raise RuntimeError("decode_nms's tensors must be contiguous, keep int32")
        a.T, a.K, a.keep_stride = T, r["boxes"].shape[0], r["keep"].shape[1]
        a.boxes, a.scores, a.labels, a.keep = _hip.ptr(r["boxes"]), _hip.ptr(r["scores"]), _hip.ptr(r["labels"]), _hip.ptr(r["keep"])
        a.keep_count, a.seg_offsets = _hip.ptr(r["keep_count"]), _hip.ptr(r["seg_offsets_device"])
        a.label_base[:T] = [int(v) for v in label_base]
        status = r["status"]
    a.status = _hip.ptr(status)
    _hip.check(_hip.lib().dal3_roi_targets(a, _hip.stream()))
    out["status"] = status
    out["roi_labels"] = out["roi_labels"].long()
    out["reg_valid_mask"] = out["reg_valid_i32"].long()
    out["rcnn_cls_labels"] = out["cls_labels_f32"].long() if kind == "cls" else out["cls_labels_f32"]
    return out


class ProposalTargetLayer(nn.Module):
    """proposal_target_layer.py on dal3_roi_targets. forward(batch_dict, draws=None, generator=None): rois (B, M, code),
    roi_scores, roi_labels, gt_boxes_and_cls (B, G, code + 1) and, optionally, roi_features (B, M, C) -> the reference's
    targets_dict (rois, gt_of_rois [the assigned GT rows, not yet encoded], gt_iou_of_rois, roi_scores, roi_labels,
    roi_features, reg_valid_mask, rcnn_cls_labels) and the kernel's other outputs under their own names (slot, sample,
    gt_of_rois_encoded, status). draws (B, M + ROI_PER_IMAGE) float32 in [0, 1) replaces the reference's NumPy / torch
    draws (include/dal3.h says how each is used); None draws torch.rand on the device."""

    def __init__(self, roi_sampler_cfg):
        super().__init__()
        self.roi_sampler_cfg = roi_sampler_cfg

    @torch.no_grad()
    def forward(self, batch_dict, draws=None, generator=None):
        rois = batch_dict["rois"]
        t = roi_targets(self.roi_sampler_cfg, rois.shape[-1], batch_dict["gt_boxes_and_cls"], draws, rois=rois,
                        roi_scores=batch_dict["roi_scores"], roi_labels=batch_dict["roi_labels"], generator=generator)
        out = {k: t[k] for k in ("rois", "gt_iou_of_rois", "roi_scores", "roi_labels", "reg_valid_mask", "rcnn_cls_labels", "slot",
                                 "sample", "status", "reg_valid_i32", "cls_labels_f32")}
        out["gt_of_rois"], out["gt_of_rois_encoded"] = t["gt_of_rois_src"], t["gt_of_rois"]
        feats = batch_dict.get("roi_features")
        if feats is not None:
            out["roi_features"] = torch.gather(feats, 1, t["slot"].long().unsqueeze(-1).expand(-1, -1, feats.shape[-1]))
        return out


class _RoILoss(torch.autograd.Function):
    """dal3_roi_loss: (rcnn_cls (N, 1), rcnn_reg (N, code)) -> loss (3): cls, reg, their sum; the gradients come out of the
    same launch"""

    @staticmethod
    def forward(ctx, rcnn_cls, rcnn_reg, cls_labels, reg_valid, gt_of_rois, code_weights, cls_weight, reg_weight):
        cls, reg = rcnn_cls.detach().contiguous().float(), rcnn_reg.detach().contiguous().float()
        N, code = reg.shape
        loss = torch.empty(3, dtype=torch.float32, device=reg.device)
        d_cls, d_reg = torch.empty_like(cls), torch.empty_like(reg)
        cw = (C.c_float * code)(*[float(v) for v in code_weights[:code]])
        _hip.check(_hip.lib().dal3_roi_loss(_hip.ptr(cls), _hip.ptr(reg), N, code, _hip.ptr(cls_labels), _hip.ptr(reg_valid),
                                            _hip.ptr(gt_of_rois), cw, float(cls_weight), float(reg_weight), _hip.ptr(loss),
                                            _hip.ptr(d_cls), _hip.ptr(d_reg), _hip.stream()))
        ctx.save_for_backward(d_cls, d_reg)
        ctx.shapes = (rcnn_cls.shape, rcnn_reg.shape)
        return loss

    @staticmethod
    def backward(ctx, g):
        d_cls, d_reg = ctx.saved_tensors
        return ((g[0] + g[2]) * d_cls).reshape(ctx.shapes[0]), ((g[1] + g[2]) * d_reg).reshape(ctx.shapes[1]), None, None, None, None, \
            None, None


class RoIHead(rpn._PackedLayers):
    """roi_head.py: shared_fc_layer, cls_layers and reg_layers as the reference builds them (the Dropout slots keep the
    Sequential indices of a checkpoint). forward(batch_dict, training=False):
    rois (B, M, code_size), roi_scores (B, M), roi_features (B, M, input_channels) -> batch_cls_preds (B, M, 1),
    batch_box_preds (B, M, code_size), cls_preds_normalized False, through dal3_roi_head's direct form.
    Training is `train_forward` (the reference's forward(training=True)), `assign_targets`, `get_loss`,
    `get_box_cls_layer_loss`, `get_box_reg_layer_loss` and `forward_ret_dict`, with the reference's keys and tb_dict names; the
    tensors, tb_dict's `rcnn_loss` included, stay on the device."""

    def __init__(self, input_channels, model_cfg, num_class=1, code_size=7, test_cfg=None):
        super().__init__()
        self.model_cfg, self.test_cfg, self.num_class, self.code_size = model_cfg, test_cfg, num_class, code_size
        self.input_channels = int(input_channels)
        shared, cls, reg = (list(_get(model_cfg, k)) for k in ("SHARED_FC", "CLS_FC", "REG_FC"))
        dp = float(_get(model_cfg, "DP_RATIO", 0))
        if num_class != 1:
            raise ValueError(f"num_class = {num_class}: the RoI head is built class-agnostic (num_class 1)")
        if code_size not in (7, 9):
            raise ValueError(f"code_size = {code_size}: 7, or 9 with the velocity")
        for name, widths in (("SHARED_FC", shared), ("CLS_FC", cls), ("REG_FC", reg)):
            if not 1 <= len(widths) <= 3 or any(w % 16 or not 16 <= w <= _hip.ROI_MAX_WIDTH for w in widths):
                raise ValueError(f"{name} = {widths}: the kernel serves 1 to 3 widths, multiples of 16 up to {_hip.ROI_MAX_WIDTH}")
        self.target_config, self.loss_config = _get(model_cfg, "TARGET_CONFIG"), _get(model_cfg, "LOSS_CONFIG")
        self.proposal_target_layer = ProposalTargetLayer(self.target_config) if self.target_config is not None else None
        self.forward_ret_dict = None
        pre, layers = self.input_channels, []
        for k, w in enumerate(shared):
            layers += [nn.Conv1d(pre, w, kernel_size=1, bias=False), nn.BatchNorm1d(w), nn.ReLU()]
            pre = w
            if k != len(shared) - 1 and dp > 0:
                layers.append(nn.Dropout(dp))
        self.shared_fc_layer = nn.Sequential(*layers)
        self.cls_layers = self.make_fc_layers(pre, self.num_class, cls, dp)
        self.reg_layers = self.make_fc_layers(pre, code_size, reg, dp)
        self.init_weights("xavier")

    @staticmethod
    def make_fc_layers(input_channels, output_channels, fc_list, dp):
        layers, pre = [], input_channels
        for k, w in enumerate(fc_list):
            layers += [nn.Conv1d(pre, w, kernel_size=1, bias=False), nn.BatchNorm1d(w), nn.ReLU()]
            pre = w
            if dp >= 0 and k == 0:
                layers.append(nn.Dropout(dp))
        layers.append(nn.Conv1d(pre, output_channels, kernel_size=1, bias=True))
        return nn.Sequential(*layers)

    def init_weights(self, weight_init="xavier"):
        init = {"kaiming": nn.init.kaiming_normal_, "xavier": nn.init.xavier_normal_, "normal": nn.init.normal_}.get(weight_init)
        if init is None:
            raise NotImplementedError(weight_init)
        for m in self.modules():
            if isinstance(m, nn.Conv1d):
                init(m.weight, mean=0, std=0.001) if weight_init == "normal" else init(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    def _plan(self):
        """[(conv, bn or None)] in dal3_roi_pack's order: shared, cls (its final layer last), reg"""
        plan = []
        for seq in (self.shared_fc_layer, self.cls_layers, self.reg_layers):
            for m in seq:
                if isinstance(m, nn.Conv1d):
                    plan.append([m, None])
                elif isinstance(m, nn.BatchNorm1d):
                    plan[-1][1] = m
        return [tuple(p) for p in plan]

    def shape(self):
        count = [sum(isinstance(m, nn.BatchNorm1d) for m in seq) for seq in (self.shared_fc_layer, self.cls_layers, self.reg_layers)]
        s = _hip.RoiShape(c_in=self.input_channels, n_shared=count[0], n_cls=count[1], n_reg=count[2], num_class=self.num_class,
                          code_size=self.code_size)
        widths = [conv.out_channels for conv, bn in self._plan() if bn is not None]
        s.shared[:count[0]] = widths[:count[0]]
        s.cls[:count[1]] = widths[count[0]:count[0] + count[1]]
        s.reg[:count[2]] = widths[count[0] + count[1]:]
        return s

    def _pack(self, plan):
        lib, shape = _hip.lib(), self.shape()
        n = len(plan)
        layers, eps = (_hip.Layer * n)(), (C.c_double * n)()
        for i, (conv, bn) in enumerate(plan):
            layers[i] = _hip.fold_layer_struct(conv, bn, "the RoI head's parameters")
            eps[i] = float(bn.eps) if bn is not None else 1e-5
        floats = lib.dal3_roi_pack_floats(shape)
        if floats == 0:
            raise RuntimeError("the RoI head's shape is not served by dal3_roi_head")
        buf = torch.empty(floats, dtype=torch.float32, device=plan[0][0].weight.device)
        _hip.check(lib.dal3_roi_pack(shape, layers, n, eps, _hip.ptr(buf), _hip.stream()))
        return buf

    def forward(self, batch_dict, training=False):
        if training or self.training:
            raise NotImplementedError("RoIHead.forward(training=True): training does not go through forward (the randomness is an "
                                      "input there): call train_forward(batch_dict, draws) in train mode, or .eval() and pass "
                                      "training=False")
        rois = _f32(batch_dict["rois"], "rois", 3)
        B, M, code = rois.shape
        if code != self.code_size:
            raise ValueError(f"rois have {code} columns, the head's code_size is {self.code_size}")
        scores = _f32(batch_dict["roi_scores"], "roi_scores", 2)
        feats = _f32(batch_dict["roi_features"], "roi_features", 3)
        if tuple(scores.shape) != (B, M) or tuple(feats.shape) != (B, M, self.input_channels):
            raise ValueError(f"roi_scores {tuple(scores.shape)} / roi_features {tuple(feats.shape)} do not match rois {tuple(rois.shape)} "
                             f"and {self.input_channels} input channels")
        batch_dict["batch_size"] = B
        with torch.no_grad():
            box = torch.empty((B, M, code), dtype=torch.float32, device=rois.device)
            cls = torch.empty((B, M, 1), dtype=torch.float32, device=rois.device)
            a = _hip.RoiHeadArgs(shape=self.shape(), packed=_hip.ptr(self.packed()), B=B, M=M, num_point=1, C=self.input_channels,
                                 rois=_hip.ptr(rois), roi_scores=_hip.ptr(scores), roi_features=_hip.ptr(feats),
                                 box_preds=_hip.ptr(box), cls_preds=_hip.ptr(cls))
            _hip.check(_hip.lib().dal3_roi_head(a, _hip.stream()))
        batch_dict["batch_cls_preds"], batch_dict["batch_box_preds"], batch_dict["cls_preds_normalized"] = cls, box, False
        return batch_dict

    # ------------------------------------------------------------------ training
    def assign_targets(self, batch_dict, draws=None, generator=None):
        """roi_head_template.py:43: ProposalTargetLayer.forward, then gt_of_rois_src (the assigned rows) and the encoded
        gt_of_rois, which dal3_roi_targets wrote in the same launch"""
        if self.proposal_target_layer is None:
            raise ValueError("model_cfg has no TARGET_CONFIG")
        t = self.proposal_target_layer(batch_dict, draws, generator)
        t["gt_of_rois_src"], t["gt_of_rois"] = t["gt_of_rois"], t.pop("gt_of_rois_encoded")
        return t

    def _segments(self):
        """each Sequential cut at its Dropout modules -> [[([(conv, bn)], final conv or None, dropout p or None)]]"""
        out = []
        for seq in (self.shared_fc_layer, self.cls_layers, self.reg_layers):
            segs, pairs, final = [], [], None
            for m in seq:
                if isinstance(m, nn.Conv1d):
                    pairs.append([m, None])
                elif isinstance(m, nn.BatchNorm1d):
                    pairs[-1][1] = m
                elif isinstance(m, nn.Dropout):
                    segs.append(([tuple(p) for p in pairs], None, m.p))
                    pairs = []
            if pairs and pairs[-1][1] is None:
                final = pairs.pop()[0]
            if pairs or final is not None:
                segs.append(([tuple(p) for p in pairs], final, None))
            out.append(segs)
        return out

    def _train_stack(self, x, segs, masks):
        from . import train
        lib = _hip.lib()
        for pairs, final, p in segs:
            params, bns = [], []
            for conv, bn in pairs:
                if bn.eps != train._EPS or bn.momentum != train._MOM or not bn.track_running_stats or not bn.affine:
                    raise NotImplementedError(f"BatchNorm1d(eps={bn.eps}, momentum={bn.momentum}): the training kernels hold {train._EPS} / "
                                              f"{train._MOM}, affine, with running statistics")
                params += [conv.weight.squeeze(-1), conv.weight.new_zeros(conv.out_channels), bn.weight, bn.bias]
                bns.append(bn)
            if final is not None:
                params += [final.weight.squeeze(-1), final.bias]
            if bns:
                with torch.no_grad():
                    torch._foreach_add_([bn.num_batches_tracked for bn in bns], 1)
            stats = [(bn.running_mean, bn.running_var) for bn in bns]
            # the rows-are-items kernels hold the input activation of every layer behind the piece's first in LDS
            behind = [conv for conv, _ in pairs][1:] + ([final] if final is not None and pairs else [])
            narrow = all(conv.in_channels <= lib.dal3_tr_fc_max_act_cin() for conv in behind)
            if train.FC_ROWS_KERNELS and narrow and 2 <= x.shape[0] <= lib.dal3_tr_fc_max_rows():
                x = train._FcTailRows.apply(x, stats, len(bns), *params)
            else:
                if x.shape[0] < 2 or any(w % 32 for conv, _ in pairs for w in (conv.in_channels, conv.out_channels)) or \
                        (final is not None and final.in_channels % 32):
                    raise NotImplementedError(f"{x.shape[0]} rows: beyond dal3_tr_fc_max_rows() = {lib.dal3_tr_fc_max_rows()} rows the "
                                              "training kernels need widths that are multiples of 32 (and at least 2 rows)")
                x = train._FcTail.apply(x, stats, len(bns), *params)
            if p is not None:
                # Dropout stays a stock torch op (train.py); an injected mask replaces the draw
                x = x * masks.pop(0) if masks is not None else F.dropout(x, p, True)
        return x

    def _train_head(self, features, targets, drop_masks=None):
        """the three stacks in train mode on the sampled rows (B, R, input_channels) -> forward_ret_dict"""
        if not self.training:
            raise RuntimeError("RoIHead.train_forward runs in train mode: call .train()")
        N = features.shape[0] * features.shape[1]
        masks = None if drop_masks is None else [_f32(m, "drop_masks[i]", 2) for m in drop_masks]
        shared, cls, reg = self._segments()
        n_drop = [sum(p is not None for _, _, p in segs) for segs in (shared, cls, reg)]
        if masks is not None and len(masks) != sum(n_drop):
            raise ValueError(f"{len(masks)} drop_masks for {sum(n_drop)} Dropout modules (shared, cls, reg in this order)")
        x = self._train_stack(features.reshape(N, -1), shared, masks)
        rcnn_cls = self._train_stack(x, cls, masks)
        rcnn_reg = self._train_stack(x, reg, masks)
        targets = dict(targets)
        targets["rcnn_cls"], targets["rcnn_reg"] = rcnn_cls, rcnn_reg
        self.forward_ret_dict = targets
        return targets

    def train_forward(self, batch_dict, draws=None, drop_masks=None, generator=None):
        """roi_head.py:70 with training=True: assign_targets, the sampled rois / labels / features put back into batch_dict,
        the three Sequential stacks in train mode (batch statistics over the B * ROI_PER_IMAGE rows, the running statistics
        and num_batches_tracked updated) as autograd Functions on the training kernels (train._FcTailRows up to
        dal3_tr_fc_max_rows() rows, train._FcTail beyond; the bias-free convolutions get a zero bias), rcnn_cls and rcnn_reg
        into forward_ret_dict. drop_masks: the Dropout multipliers (rows, width) in the order shared, cls, reg (tests)."""
        batch_dict["batch_size"] = len(batch_dict["rois"])
        if batch_dict.get("roi_features") is None:
            raise ValueError("train_forward needs batch_dict['roi_features'] (B, M, input_channels)")
        targets = self.assign_targets(batch_dict, draws, generator)
        batch_dict["rois"], batch_dict["roi_labels"], batch_dict["roi_features"] = targets["rois"], targets["roi_labels"], targets["roi_features"]
        self._train_head(targets["roi_features"], targets, drop_masks)
        return batch_dict

    def _losses(self, ret):
        cfg = self.loss_config
        if _get(cfg, "CLS_LOSS") != "BinaryCrossEntropy":
            raise NotImplementedError(f"CLS_LOSS = {_get(cfg, 'CLS_LOSS')!r}: BinaryCrossEntropy is built (dal3_roi_loss)")
        if _get(cfg, "REG_LOSS") != "L1":
            raise NotImplementedError(f"REG_LOSS = {_get(cfg, 'REG_LOSS')!r}: L1 is built (dal3_roi_loss)")
        if ret.get("_loss") is None or ret["_loss"][0] is not ret["rcnn_cls"]:
            w = _get(cfg, "LOSS_WEIGHTS")
            code = ret["rcnn_reg"].shape[-1]
            if len(w["code_weights"]) < code:
                raise ValueError(f"{len(w['code_weights'])} code_weights for code_size {code}")
            loss = _RoILoss.apply(ret["rcnn_cls"], ret["rcnn_reg"], ret["cls_labels_f32"], ret["reg_valid_i32"], ret["gt_of_rois"],
                                  list(w["code_weights"]), w["rcnn_cls_weight"], w["rcnn_reg_weight"])
            ret["_loss"] = (ret["rcnn_cls"], loss)
        return ret["_loss"][1]

    def get_box_cls_layer_loss(self, forward_ret_dict):
        loss = self._losses(forward_ret_dict)[0]
        return loss, {"rcnn_loss_cls": loss.detach()}

    def get_box_reg_layer_loss(self, forward_ret_dict):
        loss = self._losses(forward_ret_dict)[1]
        return loss, {"rcnn_loss_reg": loss.detach()}

    def get_loss(self, tb_dict=None):
        """roi_head_template.py:140 -> (rcnn_loss, tb_dict); the three losses come out of one dal3_roi_loss launch and
        tb_dict['rcnn_loss'] is a device tensor (the reference reads it back with .item())"""
        if self.forward_ret_dict is None:
            raise RuntimeError("get_loss before train_forward")
        tb_dict = {} if tb_dict is None else tb_dict
        rcnn_loss_cls, cls_tb = self.get_box_cls_layer_loss(self.forward_ret_dict)
        rcnn_loss_reg, reg_tb = self.get_box_reg_layer_loss(self.forward_ret_dict)
        rcnn_loss = self._losses(self.forward_ret_dict)[2]
        tb_dict.update(cls_tb)
        tb_dict.update(reg_tb)
        tb_dict["rcnn_loss"] = rcnn_loss.detach()
        return rcnn_loss, tb_dict


SECOND_STAGE = {"BEVFeatureExtractor": BEVFeatureExtractor}
ROI_HEADS = {"RoIHead": RoIHead}


class TwoStageDetector(nn.Module):
    """two_stage.py. first_stage_cfg: the one-stage model's dict (`type` VoxelNet or PointPillars, its own `pretrained` loads
    it); **first_stage_kwargs go to it as well (max_points, max_voxels, voxel_size, pc_range: the voxel generator `detect`
    uses). second_stage_modules: one BEVFeatureExtractor. `bbox_head` is `single_det.bbox_head`, so a reference checkpoint's
    duplicated bbox_head.* keys load with strict=True."""

    def __init__(self, first_stage_cfg, second_stage_modules, roi_head, NMS_POST_MAXSIZE, num_point=1, freeze=False, train_cfg=None,
                 test_cfg=None, pretrained=None, **first_stage_kwargs):
        super().__init__()
        from . import detector
        if _get(test_cfg, "double_flip", False):
            raise ValueError("test_cfg.double_flip with a two-stage model is refused: the reference indexes the 4 B flipped maps with "
                             "B samples there")
        if num_point not in (1, 5):
            raise NotImplementedError(f"num_point = {num_point} (1 or 5)")
        table = {"VoxelNet": detector.VoxelNet, "PointPillars": detector.PointPillars}
        if isinstance(first_stage_cfg, nn.Module):
            self.single_det = first_stage_cfg
        else:
            args = dict(first_stage_cfg)
            kind = args.pop("type")
            if kind not in table:
                raise KeyError(f"first stage type {kind!r} is not built here (known: {sorted(table)})")
            self.single_det = table[kind](**args, train_cfg=train_cfg, test_cfg=test_cfg, **first_stage_kwargs)
        self.NMS_POST_MAXSIZE, self.num_point, self.freeze = int(NMS_POST_MAXSIZE), int(num_point), bool(freeze)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.bbox_head = self.single_det.bbox_head
        self.second_stage = nn.ModuleList(detector._build(m, SECOND_STAGE, "second stage module") for m in second_stage_modules)
        if len(self.second_stage) != 1:
            raise NotImplementedError(f"{len(self.second_stage)} second stage modules: one BEVFeatureExtractor is served (the "
                                      "voxel_feature stream is not built)")
        self.roi_head = detector._build(roi_head, ROI_HEADS, "roi_head")
        self._post = None
        if pretrained is not None:
            self.init_weights(pretrained)

    def init_weights(self, pretrained):
        """a checkpoint path: its `state_dict` (or the file itself) must hold exactly this model's keys"""
        ckpt = torch.load(pretrained, map_location="cpu")
        self.load_state_dict(ckpt.get("state_dict", ckpt), strict=True)

    to_prediction = staticmethod(CenterHeadPost.to_prediction)

    @property
    def precision(self):
        """`single_det.precision`: the first stage's neck and head on 'fp32' | 'fp16' | 'bf16' MFMA operands. The BEV
        feature extractor reads the neck's float32 map as before, and the RoI head stays fp32."""
        return self.single_det.precision

    @precision.setter
    def precision(self, value):
        self.single_det.precision = value

    @property
    def sparse_precision(self):
        """`single_det.sparse_precision`: the first stage's sparse 3-D middle on 'fp32' | 'fp16' | 'bf16' MFMA operands"""
        return self.single_det.sparse_precision

    @sparse_precision.setter
    def sparse_precision(self, value):
        self.single_det.sparse_precision = value

    def post(self):
        if self._post is None or self._post[0] is not self.test_cfg:
            self._post = (self.test_cfg, CenterHeadPost(self.test_cfg, self.bbox_head.num_classes))
        return self._post[1]

    # ------------------------------------------------------------------ the reference's steps, one by one
    def get_box_center(self, boxes):
        return [box_points(box["box3d_lidar"], 1 if len(box["box3d_lidar"]) == 0 else self.num_point) for box in boxes]

    def reorder_first_stage_pred_and_feature(self, first_pred, example, features):
        B, M, cols = len(first_pred), self.NMS_POST_MAXSIZE, first_pred[0]["box3d_lidar"].shape[1]
        dev = first_pred[0]["box3d_lidar"].device
        rois = torch.zeros((B, M, cols), dtype=torch.float32, device=dev)
        roi_scores = torch.zeros((B, M), dtype=torch.float32, device=dev)
        roi_labels = torch.zeros((B, M), dtype=torch.long, device=dev)
        roi_features = torch.zeros((B, M, sum(f[0].shape[-1] for f in features)), dtype=torch.float32, device=dev)
        for i in range(B):
            n = features[0][i].shape[0]
            box = first_pred[i]["box3d_lidar"]
            if self.roi_head.code_size == 9:
                box = box[:, [0, 1, 2, 3, 4, 5, 8, 6, 7]]
            rois[i, :n] = box                   # more than M rows: torch's shape error, as in the reference
            roi_labels[i, :n] = first_pred[i]["label_preds"] + 1
            roi_scores[i, :n] = first_pred[i]["scores"]
            roi_features[i, :n] = torch.cat([f[i] for f in features], dim=-1)
        example.update(rois=rois, roi_labels=roi_labels, roi_scores=roi_scores, roi_features=roi_features, has_class_labels=True)
        return example

    def post_process(self, batch_dict):
        """two_stage.py:121 (this step reads the label mask back: it is the module-by-module route, not `forward`'s)"""
        B = batch_dict["batch_size"]
        box, cls, scores = batch_dict["batch_box_preds"].contiguous(), batch_dict["batch_cls_preds"].contiguous(), \
            batch_dict["roi_scores"].contiguous()
        M, code = box.shape[1], box.shape[2]
        out_box, out_score = torch.empty_like(box), torch.empty_like(scores)
        _hip.check(_hip.lib().dal3_roi_post(_hip.ptr(box), _hip.ptr(cls), _hip.ptr(scores), B * M, code, _hip.ptr(out_box),
                                            _hip.ptr(out_score), _hip.stream()))
        ret = []
        for i in range(B):
            label = batch_dict["roi_labels"][i]
            mask = (label != 0).reshape(-1)
            ret.append({"box3d_lidar": out_box[i][mask, :], "scores": out_score[i][mask], "label_preds": label[mask] - 1,
                        "metadata": batch_dict["metadata"][i]})
        return ret

    # ------------------------------------------------------------------ the fused device part
    @torch.no_grad()
    def refine(self, r, bev):
        """r: CenterHeadPost.decode_nms's dict; bev: the neck's (B, C, H, W) map. Enqueued, nothing read back -> a dict of
        device tensors: boxes (B, M, code_size), scores (B, M), labels (B, M) int32 (the first stage's, with the task's
        class offset), counts (B) int32, status (1) int32 (r's status OR-ed with this stage's), features (B, M,
        num_point * C); M = NMS_POST_MAXSIZE. Rows past a sample's count are zero."""
        ext, head, M, P = self.second_stage[0], self.roi_head, self.NMS_POST_MAXSIZE, self.num_point
        view = _map(bev, "NCHW", None, "bev")
        B, H, W, Cn = view.shape
        T = len(self.bbox_head.num_classes)
        if r["B"] != B or r["keep"].shape[0] != T * B:
            raise ValueError(f"the first stage's result holds {r['B']} samples in {r['keep'].shape[0]} segments, the map {B} samples")
        if P * Cn != head.input_channels:
            raise ValueError(f"num_point * C = {P} * {Cn}, the RoI head takes {head.input_channels} input channels")
        cols, code, dev = r["boxes"].shape[1], head.code_size, view.device
        if cols != code:
            raise ValueError(f"the first stage's boxes have {cols} columns, the RoI head's code_size is {code}")
        lib = _hip.lib()
        boxes = torch.zeros((B, M, code), dtype=torch.float32, device=dev)
        scores = torch.zeros((B, M), dtype=torch.float32, device=dev)
        labels = torch.zeros((B, M), dtype=torch.int32, device=dev)
        counts = torch.zeros(B, dtype=torch.int32, device=dev)
        feats = torch.zeros((B, M, P * Cn), dtype=torch.float32, device=dev)
        status = r["status"]
        nbytes = lib.dal3_roi_head_workspace_bytes(B, M, P, Cn, code)
        ws = _hip.workspace(nbytes, dev)
        a = _hip.RoiHeadArgs(shape=head.shape(), packed=_hip.ptr(head.packed()), B=B, M=M, num_point=P, C=Cn, T=T, box_cols=cols,
                             K=r["boxes"].shape[0], keep_stride=r["keep"].shape[1], boxes=_hip.ptr(r["boxes"]),
                             scores=_hip.ptr(r["scores"]), labels=_hip.ptr(r["labels"]), keep=_hip.ptr(r["keep"]),
                             keep_count=_hip.ptr(r["keep_count"]), seg_offsets=_hip.ptr(r["seg_offsets_device"]),
                             bev=_map_struct(view), H=H, W=W, out_stride=float(ext.out_stride), out_boxes=_hip.ptr(boxes),
                             out_scores=_hip.ptr(scores), out_labels=_hip.ptr(labels), out_counts=_hip.ptr(counts),
                             out_features=_hip.ptr(feats), status=_hip.ptr(status), workspace=_hip.ptr(ws), workspace_bytes=nbytes)
        a.label_base[:T] = [int(v) for v in np.concatenate([[0], np.cumsum(self.bbox_head.num_classes)[:-1]])]
        a.pc_start[:] = [float(v) for v in ext.pc_start[:2]]
        a.voxel_size[:] = [float(v) for v in ext.voxel_size[:2]]
        if not (r["keep"].is_contiguous() and r["boxes"].is_contiguous() and r["keep"].dtype == torch.int32):
            raise RuntimeError("decode_nms's tensors must be contiguous, keep int32")
        if B:
            _hip.check(lib.dal3_roi_head(a, _hip.stream()))
        return {"boxes": boxes, "scores": scores, "labels": labels, "counts": counts, "status": status, "features": feats}

    # ------------------------------------------------------------------ the second stage's training
    def roi_loss(self, r, bev, gt_boxes_and_cls, draws=None, drop_masks=None):
        """the device part of a training step, like `refine`: r (decode_nms's dict) and bev (the neck's (B, C, H, W) map), both
        without gradient, and gt_boxes_and_cls (B, G, code_size + 1) -> {"loss" (the RoI loss, with the graph of every
        roi_head.* parameter behind it), "roi_cls_loss", "roi_reg_loss" (detached), "status", "targets" (forward_ret_dict)}.
        dal3_roi_targets' fused form, dal3_box_points and dal3_bev_gather of the ROI_PER_IMAGE sampled rows alone (zero rows for empty slots),
        the head's stacks in train mode, dal3_roi_loss: enqueued on one stream, nothing read back."""
        ext, head, M, P = self.second_stage[0], self.roi_head, self.NMS_POST_MAXSIZE, self.num_point
        with torch.no_grad():
            view = _map(bev.detach(), "NCHW", None, "bev")
            B, H, W, Cn = view.shape
            if P * Cn != head.input_channels:
                raise ValueError(f"num_point * C = {P} * {Cn}, the RoI head takes {head.input_channels} input channels")
            base = [int(v) for v in np.concatenate([[0], np.cumsum(self.bbox_head.num_classes)[:-1]])]
            t = roi_targets(head.target_config, head.code_size, gt_boxes_and_cls, draws, fused=(r, base), M=M)
            R = t["slot"].shape[1]
            n = B * R
            feats = torch.zeros((B, R, P * Cn), dtype=torch.float32, device=view.device)
            # the module route's own two kernels on the R sampled boxes (the bits of refine's rows, tests/test_gpu_roi.py):
            # the kernel's rotation-last copy of the rois for dal3_box_points; dal3_bev_gather skips the empty slots' sample -1 over the zeroed rows
            pts = box_points(t["boxes"].reshape(n, -1), P)
            sample = t["sample"].reshape(-1)
            for p in range(P if n else 0):
                a = ext._args(view)
                sec = pts[p * n:(p + 1) * n]
                a.n, a.xy, a.xy_stride, a.sample, a.sample_index = n, _hip.ptr(sec), pts.stride(0), _hip.ptr(sample), 0
                a.points_per_row, a.out, a.out_row_stride, a.out_col_offset = 1, _hip.ptr(feats), P * Cn, p * Cn
                _hip.check(_hip.lib().dal3_bev_gather(a, _hip.stream()))
            t["roi_features"] = feats
        head._train_head(feats, t, drop_masks)
        loss, tb = head.get_loss()
        return {"loss": loss, "roi_cls_loss": tb["rcnn_loss_cls"], "roi_reg_loss": tb["rcnn_loss_reg"], "status": t["status"],
                "targets": head.forward_ret_dict}

    def second_stage_loss(self, example, draws=None):
        """two_stage.py's forward(return_loss=True) under `freeze`: the first stage through its eval route without gradient (the
        reference's FrozenBatchNorm2d is the folded eval BatchNorm), the RoI head in train mode -> {"loss": [rcnn_loss],
        "roi_reg_loss": [...], "roi_cls_loss": [...]}. example: forward's keys and gt_boxes_and_cls (B, G, 10: with code_size 7
        the columns [0..6, -1] are taken, as in the reference). Deviation: the one-stage loss terms that the reference's
        combine_loss adds carry no gradient under `freeze`; they are not computed, so `loss` holds the RoI loss alone."""
        if not self.freeze:
            raise NotImplementedError("second_stage_loss with freeze=False: the first stage's loss and training are not built; only "
                                      "the frozen first stage (freeze=True) is served")
        if not self.roi_head.training:
            raise RuntimeError("second_stage_loss trains the RoI head: call roi_head.train() (and keep single_det in eval mode)")
        det = self.single_det
        if det.training:
            raise RuntimeError("the frozen first stage runs its eval route: call single_det.eval()")
        with torch.no_grad():
            data = dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"],
                        batch_size=len(example["num_voxels"]), input_shape=example["shape"][0])
            x = det.extract_feat(data)
            x = x[0] if isinstance(x, tuple) else x
            r = self.post().decode_nms(self.bbox_head(x))
            gt = example["gt_boxes_and_cls"]
            if self.roi_head.code_size == 7:
                gt = gt[:, :, [0, 1, 2, 3, 4, 5, 6, -1]]
        out = self.roi_loss(r, x, gt.contiguous(), draws)
        self.last_roi_loss = out
        return {"loss": [out["loss"]], "roi_reg_loss": [out["roi_reg_loss"]], "roi_cls_loss": [out["roi_cls_loss"]]}

    def _finish(self, out, metadata):
        """the one host synchronisation: counts and status -> post_process's list"""
        B = out["counts"].shape[0]
        if metadata is not None and len(metadata) != B:
            raise ValueError(f"{len(metadata)} metadata entries for {B} samples")
        host = torch.cat([out["counts"], out["status"]]).cpu().numpy()
        st = int(host[-1])
        if st & _hip.ROI_OVERFLOW:
            raise RuntimeError(f"a sample's first stage kept more boxes than NMS_POST_MAXSIZE = {self.NMS_POST_MAXSIZE} (status "
                               "DAL3_ROI_OVERFLOW; the reference raises a shape error): raise it, or lower nms_post_max_size")
        CenterHeadPost.check_status(torch.from_numpy(host[-1:]))
        ret = []
        for i in range(B):
            n = int(host[i])
            ret.append({"box3d_lidar": out["boxes"][i, :n], "scores": out["scores"][i, :n],
                        "label_preds": out["labels"][i, :n].to(torch.int64), "metadata": None if metadata is None else metadata[i]})
        return ret

    def _refuse(self, return_loss):
        if return_loss:
            raise NotImplementedError("TwoStageDetector.forward(return_loss=True): the detector's loss is not built; this is the "
                                      "eval-mode detector (call with return_loss=False; the second stage's loss on a frozen first "
                                      "stage is second_stage_loss)")
        if self.training:
            raise RuntimeError("the two-stage detector is the eval-mode route: call .eval()")

    def _second(self, x, metadata):
        r = self.post().decode_nms(self.bbox_head(x))
        self.last_refine = self.refine(r, x)
        return self._finish(self.last_refine, metadata)

    @torch.no_grad()
    def forward(self, example, return_loss=False, **kwargs):
        self._refuse(return_loss)
        det = self.single_det
        data = dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"],
                    batch_size=len(example["num_voxels"]), input_shape=example["shape"][0])
        x = det.extract_feat(data)
        return self._second(x[0] if isinstance(x, tuple) else x, example.get("metadata"))

    @torch.no_grad()
    def detect(self, points, point_offsets, metadata=None, point_offsets_device=None):
        """the one-stage models' `detect` with the second stage behind it: points (N, C) float32 CUDA, point_offsets (B + 1)
        on the host -> post_process's list; one host synchronisation, at the end"""
        self._refuse(False)
        from . import detector
        det = self.single_det
        r = det._voxelize(points, point_offsets, point_offsets_device)
        grid = pillars.grid_size(det.voxel_size, det.pc_range)
        if isinstance(det, detector.VoxelNet):
            data = dict(features=r.voxels, num_voxels=r.num_points, coors=r.coordinates, batch_size=r.B,
                        input_shape=[int(g) for g in grid])
            x, _ = det.extract_feat(data, n_voxels=r.n_pillars)
        else:
            x = det.neck(det.reader.forward_canvas(r.voxels, r.num_points, r.coordinates, r.B, [int(grid[0]), int(grid[1])],
                                                   n_pillars=r.n_pillars))
        return self._second(x, metadata)
