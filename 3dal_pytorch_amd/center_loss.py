"""The first stage's training targets and loss on the GPU through lib3dal_hip.so (dal3_center_targets, dal3_center_loss,
include/dal3.h), under the reference's names: `AssignLabel` (det3d/datasets/pipelines/preprocess.py, the train branch),
`FastFocalLoss` and `RegLoss` (det3d/models/losses/centernet_loss.py). `rpn.CenterHead.loss` stands on `head_loss`.

The reference assigns the targets in its data pipeline, per sample, in NumPy loops on the host; here they are made from
the collated `gt_boxes_and_cls` (B, G, 10) for every sample and task in one launch, and nothing is read back. The
pipeline builds that tensor by flattening the per-task boxes, so its rows are in task order, then class order, then
original order: the slot of a row is its rank among the rows of its task, which is the reference's `k`.
"""
import numpy as np
import torch
from torch import nn

from . import _hip

REG_HEADS = ("reg", "height", "dim", "vel", "rot")
HEAD_CHANNELS = {"reg": 2, "height": 1, "dim": 3, "vel": 2, "rot": 2}


def _get(cfg, key, *default):
    if isinstance(cfg, dict):
        return cfg[key] if not default or key in cfg else default[0]
    return getattr(cfg, key, *default)


def center_targets(gt_boxes_and_cls, num_classes, pc_range, voxel_size, out_size_factor, map_size, gaussian_overlap=0.1,
                   max_objs=500, min_radius=2):
    """AssignLabel's train branch for a collated batch.

    gt_boxes_and_cls (B, G, 10) float32 CUDA: x, y, z, w, l, h, rot, vx, vy, class (1-based over all tasks; zero rows are
    padding). num_classes: the classes of every task. pc_range / voxel_size: at least their x, y entries, rounded to
    float32 as the reference's voxeliser holds them. map_size: (H, W) of the head's maps.
    -> {'hm': [...], 'anno_box': [...], 'ind': [...], 'mask': [...], 'cat': [...]}, one entry per task, with the
    reference's dtypes (float32, float32, int64, uint8, int64), and 'status': an int32 device tensor whose bit
    _hip.CENTER_OVERFLOW says that a task had more than max_objs rows (the reference asserts). One launch on the current
    stream; nothing is read back."""
    gt = gt_boxes_and_cls
    if not torch.is_tensor(gt):
        raise TypeError("gt_boxes_and_cls must be a tensor")
    _hip.require_gpu(gt, "gt_boxes_and_cls")
    if gt.dim() != 3 or gt.shape[2] != 10 or gt.dtype != torch.float32 or gt.shape[1] < 1:
        raise ValueError(f"gt_boxes_and_cls must be float32 (B, G >= 1, 10), got {gt.dtype} {tuple(gt.shape)}")
    num_classes = [int(c) for c in num_classes]
    if not 1 <= len(num_classes) <= _hip.ROI_MAX_TASKS or min(num_classes) < 1 or max(num_classes) > _hip.CENTER_MAX_CLASSES:
        raise ValueError(f"num_classes {num_classes}: 1 .. {_hip.ROI_MAX_TASKS} tasks of 1 .. {_hip.CENTER_MAX_CLASSES} classes")
    max_objs, min_radius = int(max_objs), int(min_radius)
    if not 1 <= max_objs <= _hip.CENTER_MAX_OBJS:
        raise ValueError(f"max_objs = {max_objs}: 1 .. {_hip.CENTER_MAX_OBJS}")
    H, W = (int(v) for v in map_size)
    gt = gt.contiguous()
    B, G, dev = gt.shape[0], gt.shape[1], gt.device
    out = {k: [] for k in ("hm", "anno_box", "ind", "mask", "cat")}
    for c in num_classes:
        out["hm"].append(torch.empty((B, c, H, W), dtype=torch.float32, device=dev))
        out["anno_box"].append(torch.empty((B, max_objs, 10), dtype=torch.float32, device=dev))
        out["ind"].append(torch.empty((B, max_objs), dtype=torch.int64, device=dev))
        out["mask"].append(torch.empty((B, max_objs), dtype=torch.uint8, device=dev))
        out["cat"].append(torch.empty((B, max_objs), dtype=torch.int64, device=dev))
    out["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
    a = _hip.CenterTargetsArgs(B=B, G=G, H=H, W=W, T=len(num_classes), max_objs=max_objs, gt=_hip.ptr(gt),
                               out_size_factor=float(out_size_factor), min_radius=min_radius,
                               gaussian_overlap=float(gaussian_overlap), status=_hip.ptr(out["status"]))
    for i in range(2):
        a.pc_start[i], a.voxel_size[i] = float(np.float32(pc_range[i])), float(np.float32(voxel_size[i]))
    for t, c in enumerate(num_classes):
        a.num_class[t] = c
        for k in ("hm", "anno_box", "ind", "mask", "cat"):
            getattr(a, k)[t] = out[k][t].data_ptr()
    _hip.check(_hip.lib().dal3_center_targets(a, _hip.stream()))
    return out


class AssignLabel:
    """preprocess.py's AssignLabel with the reference's constructor keys (cfg.out_size_factor, cfg.target_assigner.tasks,
    cfg.gaussian_overlap, cfg.max_objs, cfg.min_radius). The reference reads the grid from the sample it is called on;
    here `voxels` (the voxeliser's entry: shape, range, size) is given once to the constructor or with each call. Called
    on the collated `gt_boxes_and_cls`, it returns center_targets' dictionary."""

    def __init__(self, voxels=None, **kwargs):
        cfg = kwargs["cfg"]
        self.out_size_factor = _get(cfg, "out_size_factor")
        self.tasks = _get(_get(cfg, "target_assigner"), "tasks")
        self.gaussian_overlap = _get(cfg, "gaussian_overlap")
        self._max_objs = _get(cfg, "max_objs")
        self._min_radius = _get(cfg, "min_radius")
        self.voxels = voxels

    @property
    def num_classes(self):
        return [int(_get(t, "num_class", None) or len(_get(t, "class_names"))) for t in self.tasks]

    def __call__(self, gt_boxes_and_cls, voxels=None):
        voxels = self.voxels if voxels is None else voxels
        if voxels is None:
            raise ValueError("AssignLabel needs the voxeliser's `voxels` (shape, range, size), at construction or with the call")
        grid = np.asarray(_get(voxels, "shape"))
        fm = grid[:2] // self.out_size_factor       # (W, H), as the reference has it
        return center_targets(gt_boxes_and_cls, self.num_classes, _get(voxels, "range"), _get(voxels, "size"), self.out_size_factor,
                              (int(fm[1]), int(fm[0])), self.gaussian_overlap, self._max_objs, self._min_radius)


def _check_targets(hm, target_hm, anno_box, ind, mask, cat):
    B, Cc, H, W = hm.shape
    n = ind.shape[1] if ind.dim() == 2 else -1
    want = ((target_hm, torch.float32, (B, Cc, H, W), "hm"), (anno_box, torch.float32, (B, n, 10), "anno_box"),
            (ind, torch.int64, (B, n), "ind"), (mask, torch.uint8, (B, n), "mask"), (cat, torch.int64, (B, n), "cat"))
    for t, dtype, shape, name in want:
        if t is None:
            continue
        _hip.require_gpu(t, f"the target {name}")
        if t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(f"the target {name} must be {dtype} {shape}, got {t.dtype} {tuple(t.shape)}")
    if not 1 <= n <= _hip.CENTER_MAX_OBJS:
        raise ValueError(f"max_objs = {n}: 1 .. {_hip.CENTER_MAX_OBJS}")
    return n


def _launch(maps, target_hm, anno_box, ind, mask, cat, code_weights, weight):
    """dal3_center_loss on one task. maps: {'hm', 'reg', 'height', 'dim', 'rot', ['vel']} of logical (B, c, H, W) float32
    CUDA tensors of any batch / channel / row strides (a map whose W stride is not 1 is made contiguous)
    -> out (4 + n_cols): loss, hm_loss, loc_loss, num_pos, loc_loss_elem; grad (B, C + n_cols, H, W)"""
    names = [h for h in REG_HEADS if h in maps]
    ts = {}
    for name in ["hm"] + names:
        t = maps[name].detach()
        _hip.require_gpu(t, f"the head map {name}")
        if t.dim() != 4 or t.dtype != torch.float32:
            raise ValueError(f"the head map {name} must be float32 (B, C, H, W), got {t.dtype} {tuple(t.shape)}")
        ts[name] = t if t.stride(3) == 1 else t.contiguous()
    hm = ts["hm"]
    B, Cc, H, W = hm.shape
    for name in names:
        if tuple(ts[name].shape) != (B, HEAD_CHANNELS[name], H, W):
            raise ValueError(f"the head map {name} must be {(B, HEAD_CHANNELS[name], H, W)}, got {tuple(ts[name].shape)}")
    n_cols = 10 if "vel" in ts else 8
    cw = [float(v) for v in code_weights]
    if len(cw) != n_cols:
        raise ValueError(f"code_weights has {len(cw)} entries, the heads {names} make {n_cols} columns")
    n = _check_targets(hm, target_hm, anno_box, ind, mask, cat)
    if B < 1:
        raise ValueError("an empty batch has no loss")
    # the contiguous targets live until the call returns: a temporary's block could be handed to the next one
    target_hm, anno_box, ind, mask, cat = (t.contiguous() for t in (target_hm, anno_box, ind, mask, cat))
    dev = hm.device
    out = torch.empty(4 + n_cols, dtype=torch.float32, device=dev)
    grad = torch.empty((B, Cc + n_cols, H, W), dtype=torch.float32, device=dev)
    lib = _hip.lib()
    ws = _hip.workspace(lib.dal3_center_loss_workspace_bytes(B, Cc, H, W), dev)
    a = _hip.CenterLossArgs(B=B, H=H, W=W, C=Cc, n_cols=n_cols, max_objs=n, hm=_hip.nchw_map(hm), reg=_hip.nchw_map(ts["reg"]),
                            height=_hip.nchw_map(ts["height"]), dim=_hip.nchw_map(ts["dim"]), rot=_hip.nchw_map(ts["rot"]),
                            target_hm=_hip.ptr(target_hm), anno_box=_hip.ptr(anno_box), ind=_hip.ptr(ind), mask=_hip.ptr(mask),
                            cat=_hip.ptr(cat),
                            weight=float(weight), out=_hip.ptr(out), grad=_hip.ptr(grad), workspace=_hip.ptr(ws),
                            workspace_bytes=ws.numel())
    if "vel" in ts:
        a.vel = _hip.nchw_map(ts["vel"])
    for i, v in enumerate(cw):
        a.code_weights[i] = v
    _hip.check(lib.dal3_center_loss(a, _hip.stream()))
    return out, grad


class _HeadLoss(torch.autograd.Function):
    """dal3_center_loss on one task: the maps in the order hm, reg, height, dim, [vel], rot -> out (4 + n_cols). The
    gradients of out[0] (`loss`) come out of the forward launch; backward scales them. The other entries carry none."""

    @staticmethod
    def forward(ctx, names, targets, code_weights, weight, *maps):
        out, grad = _launch(dict(zip(names, maps)), *targets, code_weights, weight)
        ctx.save_for_backward(grad)
        ctx.channels = [m.shape[1] for m in maps]
        return out

    @staticmethod
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        parts = torch.split(grad * g[0], ctx.channels, dim=1)
        return (None, None, None, None) + tuple(parts)


def head_loss(preds_dict, target_hm, anno_box, ind, mask, cat, code_weights, weight):
    """one task of CenterHead.loss -> (loss, hm_loss, loc_loss, loc_loss_elem (n_cols), num_positive), device scalars;
    `loss` is differentiable in every map of preds_dict, which is read in place and not changed"""
    names = ["hm"] + [h for h in REG_HEADS if h in preds_dict]
    out = _HeadLoss.apply(names, (target_hm, anno_box, ind, mask, cat), list(code_weights), weight, *[preds_dict[k] for k in names])
    d = out.detach()
    return out[0], d[1], d[2], d[4:], d[3]


class FastFocalLoss(nn.Module):
    """centernet_loss.py's FastFocalLoss: forward(out, target, ind, mask, cat) with `out` (B, C, H, W) the clamped sigmoid
    of the heat map, as the reference passes it. The kernel takes logits, so `out` is taken back through log(out / (1 -
    out)); CenterHead.loss does not go through this module and reads the raw logits. Returns the loss alone, a device
    scalar without a graph (the gradients are CenterHead.loss's)."""

    def forward(self, out, target, ind, mask, cat):
        B, Cc, H, W = out.shape
        x = torch.logit(out.detach().float())
        zeros = {h: torch.zeros((B, HEAD_CHANNELS[h], H, W), dtype=torch.float32, device=out.device) for h in ("reg", "height", "dim", "rot")}
        box = torch.zeros((B, ind.shape[1], 10), dtype=torch.float32, device=out.device)
        res, _ = _launch(dict(hm=x, **zeros), target, box, ind, mask, cat, [0.0] * 8, 0.0)
        return res[1]


class RegLoss(nn.Module):
    """centernet_loss.py's RegLoss: forward(output (B, dim, H, W), mask, ind, target (B, max_objs, dim)) -> (dim) per-column
    L1 over mask.sum() + 1e-4, for dim 8 or 10 in the order reg, height, dim, [vel], rot. A device tensor without a graph."""

    def forward(self, output, mask, ind, target):
        B, D, H, W = output.shape
        if D not in (8, 10):
            raise ValueError(f"RegLoss takes the 8 or 10 columns of reg, height, dim, [vel], rot, got {D}")
        o = output.detach().float()
        maps = dict(hm=torch.zeros((B, 1, H, W), dtype=torch.float32, device=o.device), reg=o[:, 0:2], height=o[:, 2:3], dim=o[:, 3:6],
                    rot=o[:, D - 2:D])
        if D == 10:
            maps["vel"] = o[:, 6:8]
        box = target.float()
        if D == 8:
            box = torch.cat((box[..., :6], torch.zeros_like(box[..., :2]), box[..., 6:]), -1)
        cat = torch.zeros_like(ind)
        res, _ = _launch(maps, torch.zeros_like(maps["hm"]), box.contiguous(), ind, mask, cat, [1.0] * D, 1.0)
        return res[4:]
