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
device code and give the same bits. The second stage's training (ProposalTargetLayer, the RoI losses, `freeze`'s effect
on gradients), double-flip, the `voxel_feature` stream and num_class > 1 are not built; each is refused by name.
"""
import ctypes as C

import numpy as np
import torch
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


class RoIHead(rpn._PackedLayers):
    """roi_head.py: shared_fc_layer, cls_layers and reg_layers as the reference builds them (the Dropout slots keep the
    Sequential indices of a checkpoint), TARGET_CONFIG and LOSS_CONFIG kept and unused. forward(batch_dict, training=False):
    rois (B, M, code_size), roi_scores (B, M), roi_features (B, M, input_channels) -> batch_cls_preds (B, M, 1),
    batch_box_preds (B, M, code_size), cls_preds_normalized False, through dal3_roi_head's direct form."""

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
            for t in list(conv.parameters()) + (list(bn.parameters()) + [bn.running_mean, bn.running_var] if bn is not None else []):
                _hip.require_gpu(t, "the RoI head's parameters")
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise RuntimeError("weights must be contiguous fp32")
            layers[i] = _hip.layer_struct(conv, bn)
            eps[i] = float(bn.eps) if bn is not None else 1e-5
        floats = lib.dal3_roi_pack_floats(shape)
        if floats == 0:
            raise RuntimeError("the RoI head's shape is not served by dal3_roi_head")
        buf = torch.empty(floats, dtype=torch.float32, device=plan[0][0].weight.device)
        _hip.check(lib.dal3_roi_pack(shape, layers, n, eps, _hip.ptr(buf), _hip.stream()))
        return buf

    def forward(self, batch_dict, training=False):
        if training or self.training:
            raise NotImplementedError("RoIHead.forward(training=True): the second stage's training (ProposalTargetLayer, the RoI "
                                      "losses) is not built; call .eval() and pass training=False")
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
                                      "eval-mode detector (call with return_loss=False)")
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
