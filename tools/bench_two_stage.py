#!/usr/bin/env python3
"""Measure CenterPoint's second stage (3dal_pytorch_amd/two_stage.py, dal3_roi_head) and write
profiles/bench_two_stage.json:

    python tools/bench_two_stage.py [--batches 1 4] [--iters 30] [--warmup 5] [--points 180000] [--out profiles/bench_two_stage.json]

Two measurements.

`refine` alone: B in --batches, NMS_POST_MAXSIZE 500, a 512 x 188 x 188 BEV map (the neck's NCHW tensor), 5 points a box, the
production widths (2560 -> 256, 256 | 256, 256 -> 1 | 256, 256 -> 9), every slot of every sample in use: the fused route
(slot resolution, box points, BEV gather, MLP, box prediction, post-processing: three launches) beside the BASELINE, the
reference's formulation in stock PyTorch-ROCm ops on the same GPU and the same inputs: `permute(0, 2, 3, 1).contiguous()`
of the map, get_box_center, the indexed bilinear interpolation, the sections' `cat`, the padded rois,
Conv1d + BatchNorm1d (eval) + ReLU from the same modules, generate_predicted_boxes and post_process without its mask
(the first stage's list is given to it on the device, so it has no read-back either). HIP events around the enqueued
work; every shape warmed; the two alternate inside one process, `--iters` times; the median and the spread (min, max)
of each are recorded, and the largest difference between their outputs. No ratio is fixed in advance.

`TwoStageDetector.detect` beside `VoxelNet.detect` on tools/bench_sparse.py's sweep (random weights, wall clock around
calls that end in their read-back), B = 1, alternating: what the second stage adds to the detector end to end."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_sparse as S  # noqa: E402

two_stage = importlib.import_module("3dal_pytorch_amd.two_stage")
detector = importlib.import_module("3dal_pytorch_amd.detector")

M, P, C, HW, CODE = 500, 5, 512, 188, 9
MODEL_CFG = dict(CLASS_AGNOSTIC=True, SHARED_FC=[256, 256], CLS_FC=[256, 256], REG_FC=[256, 256], DP_RATIO=0.3, TARGET_CONFIG={},
                 LOSS_CONFIG={})
EXTRACTOR = dict(type="BEVFeatureExtractor", pc_start=[-75.2, -75.2], voxel_size=[0.1, 0.1], out_stride=8)
TASKS = [dict(num_class=3, class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"])]


class _First(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.bbox_head = torch.nn.Identity()
        self.bbox_head.num_classes = [3]


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def first_stage(B, dev, seed=0):
    """a decode_nms dictionary with M kept rows in every sample, boxes across the map and a little beyond it"""
    g = torch.Generator().manual_seed(seed)
    cap = 4096
    K = B * cap
    xy = (torch.rand((K, 2), generator=g) * 1.04 - 0.52) * 150.4
    boxes = torch.cat([xy, torch.rand((K, 1), generator=g) * 2 - 1, torch.rand((K, 3), generator=g) * 4 + 0.5,
                       torch.rand((K, 2), generator=g) * 10 - 5, (torch.rand((K, 1), generator=g) * 2 - 1) * np.pi], 1)
    keep = torch.stack([torch.randperm(cap, generator=g)[:M] for _ in range(B)]).to(torch.int32)
    off = np.arange(B + 1, dtype=np.int64) * cap
    return {"boxes": boxes.to(dev), "scores": (torch.rand(K, generator=g) * 0.8 + 0.1).to(dev),
            "labels": torch.randint(0, 3, (K,), generator=g, dtype=torch.int32).to(dev), "keep": keep.to(dev).contiguous(),
            "keep_count": torch.full((B,), M, dtype=torch.int32, device=dev), "seg_offsets": off,
            "seg_offsets_device": torch.from_numpy(off).to(dev), "status": torch.zeros(1, dtype=torch.int32, device=dev), "B": B}


def stock(m, r, bev):
    """the reference's formulation in stock ops, from the first stage's per-sample tensors on the device"""
    head, ext, B = m.roi_head, m.second_stage[0], r["B"]
    rows = r["keep"].long() + r["seg_offsets_device"][:B, None]
    nhwc = bev.permute(0, 2, 3, 1).contiguous()
    rois = torch.zeros((B, M, CODE), dtype=torch.float32, device=bev.device)
    feats = torch.zeros((B, M, P * C), dtype=torch.float32, device=bev.device)
    norm = torch.tensor([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]], device=bev.device)
    for b in range(B):
        box = r["boxes"][rows[b]]
        corners = box[:, 3:5].view(-1, 1, 2) * norm.view(1, 4, 2)
        s, c = torch.sin(box[:, -1]), torch.cos(box[:, -1])
        corners = torch.einsum("aij,jka->aik", corners, torch.stack([torch.stack([c, -s]), torch.stack([s, c])])) + box[:, :2].view(-1, 1, 2)
        mids = [(corners[:, i] + corners[:, j]) / 2 for i, j in ((0, 1), (2, 3), (0, 3), (1, 2))]
        pts = torch.cat([box[:, :2]] + mids, 0)
        x = (pts[:, 0] - ext.pc_start[0]) / ext.voxel_size[0] / ext.out_stride
        y = (pts[:, 1] - ext.pc_start[1]) / ext.voxel_size[1] / ext.out_stride
        im = nhwc[b]
        x0, y0 = torch.floor(x).long(), torch.floor(y).long()
        x1, y1 = x0 + 1, y0 + 1
        x0, x1 = torch.clamp(x0, 0, im.shape[1] - 1), torch.clamp(x1, 0, im.shape[1] - 1)
        y0, y1 = torch.clamp(y0, 0, im.shape[0] - 1), torch.clamp(y1, 0, im.shape[0] - 1)
        wa, wb = (x1.type_as(x) - x) * (y1.type_as(y) - y), (x1.type_as(x) - x) * (y - y0.type_as(y))
        wc, wd = (x - x0.type_as(x)) * (y1.type_as(y) - y), (x - x0.type_as(x)) * (y - y0.type_as(y))
        f = torch.t(torch.t(im[y0, x0]) * wa) + torch.t(torch.t(im[y1, x0]) * wb) + torch.t(torch.t(im[y0, x1]) * wc) + \
            torch.t(torch.t(im[y1, x1]) * wd)
        n = f.shape[0] // P
        feats[b] = torch.cat([f[i * n:(i + 1) * n] for i in range(P)], 1)
        rois[b] = box[:, [0, 1, 2, 3, 4, 5, 8, 6, 7]]
    scores = r["scores"][rows]
    shared = head.shared_fc_layer(feats.reshape(-1, 1, P * C).permute(0, 2, 1).contiguous())
    cls = head.cls_layers(shared).transpose(1, 2).contiguous().squeeze(1)
    reg = head.reg_layers(shared).transpose(1, 2).contiguous().squeeze(1)
    ry = rois[:, :, 6].reshape(-1)
    local = rois.clone()
    local[:, :, 0:3] = 0
    pred = (reg.view(B, M, CODE) + local).view(-1, CODE)
    cs, sn, z, o = torch.cos(ry), torch.sin(ry), torch.zeros_like(ry), torch.ones_like(ry)
    rot = torch.stack((cs, -sn, z, sn, cs, z, z, z, o), dim=1).view(-1, 3, 3)
    pred = torch.cat((torch.matmul(pred[:, None, 0:3], rot)[:, 0], pred[:, 3:]), -1)
    pred[:, 0:3] += rois[:, :, 0:3].reshape(-1, 3)
    out = pred.view(B, M, CODE)[:, :, [0, 1, 2, 3, 4, 5, 7, 8, 6]]
    return out, torch.sqrt(torch.sigmoid(cls).reshape(B, M) * scores)


def bench_refine(B, a, dev):
    torch.manual_seed(1)
    head = two_stage.RoIHead(P * C, MODEL_CFG, code_size=CODE)
    for mod in head.modules():                  # BatchNorm statistics away from (0, 1)
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.uniform_(-0.3, 0.3)
            mod.running_var.uniform_(0.5, 2.0)
    m = two_stage.TwoStageDetector(_First(), [EXTRACTOR], head, M, num_point=P).to(dev).eval()
    bev = torch.relu(torch.randn((B, C, HW, HW), device=dev))
    r = first_stage(B, dev)
    with torch.no_grad():
        for _ in range(a.warmup):
            fused, base = m.refine(r, bev), stock(m, r, bev)
        torch.cuda.synchronize()
        assert int(fused["status"].item()) == 0 and fused["counts"].tolist() == [M] * B
        diff = {"boxes_max_abs": float((fused["boxes"] - base[0]).abs().max()), "scores_max_abs": float((fused["scores"] - base[1]).abs().max()),
                "boxes_max": float(base[0].abs().max())}
        t_fused, t_base = [], []
        for _ in range(a.iters):
            t_fused.append(event_ms(lambda: m.refine(r, bev))[0])
            t_base.append(event_ms(lambda: stock(m, r, bev))[0])
    flop = 2 * B * M * (2560 * 256 + 256 * 256 * 5 + 256 * 10)
    row = {"B": B, "rows": B * M, "fused": stats(t_fused), "stock_pytorch": stats(t_base), "mlp_gflop": flop / 1e9,
           "fused_over_stock": float(np.median(t_fused) / np.median(t_base)), "difference": diff}
    return row


def bench_detect(a, dev):
    pts = S.cloud(a.points, 100)
    off = np.asarray([0, a.points], np.int64)
    dpts, doff = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    test_cfg = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0], nms=dict(nms_pre_max_size=4096, nms_post_max_size=500,
                    nms_iou_threshold=0.7), score_threshold=0.1, pc_range=list(S.RANGE[:2]), out_size_factor=8, voxel_size=list(S.VOXEL[:2]))
    first = dict(type="VoxelNet", reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5),
                 backbone=dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8),
                 neck=dict(type="RPN", layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[128, 256], us_layer_strides=[1, 2],
                           us_num_filters=[256, 256], num_input_features=256),
                 bbox_head=dict(type="CenterHead", in_channels=512, tasks=TASKS, dataset="waymo", weight=2, code_weights=[1.0] * 8,
                                common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2)}))
    torch.manual_seed(0)
    m = two_stage.TwoStageDetector(first, [EXTRACTOR], dict(type="RoIHead", input_channels=P * C, model_cfg=MODEL_CFG, code_size=7), M,
                                   num_point=P, test_cfg=test_cfg, max_points=S.MAX_POINTS, max_voxels=S.MAX_VOXELS, voxel_size=S.VOXEL,
                                   pc_range=S.RANGE).to(dev).eval()
    one = m.single_det
    # the strided levels' capacities from a first, unmeasured pass with the safe bounds, plus a tenth (as bench_sparse.py)
    grid = [int(g) for g in S.pillars.grid_size(S.VOXEL, S.RANGE)]
    r = S.pillars.voxelize(dpts, off, S.VOXEL, S.RANGE, S.MAX_POINTS, S.MAX_VOXELS, point_offsets_device=doff)
    with torch.no_grad():
        _, levels = one.backbone(one.reader(r.voxels, r.num_points, n_pillars=r.n_pillars), r.coordinates, 1, grid, n_voxels=r.n_pillars)
    caps = {k: int(int(levels[k].n.item()) * 1.1) + 32 for k in ("conv2", "conv3", "conv4")}
    caps["extra_conv"] = caps["conv4"]
    one.sparse_capacities = caps
    del levels, r

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    t_one, t_two, kept = [], [], None
    for i in range(a.warmup + a.iters):
        ms1, o1 = wall(lambda: one.detect(dpts, off, point_offsets_device=doff))
        ms2, o2 = wall(lambda: m.detect(dpts, off, point_offsets_device=doff))
        kept = [int(o["scores"].numel()) for o in o2]
        assert kept == [int(o["scores"].numel()) for o in o1]
        if i >= a.warmup:
            t_one.append(ms1)
            t_two.append(ms2)
    return {"B": 1, "points": a.points, "kept_boxes": kept, "voxelnet_detect": stats(t_one), "two_stage_detect": stats(t_two),
            "second_stage_adds_ms": float(np.median(t_two) - np.median(t_one))}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--points", type=int, default=180000)
    p.add_argument("--skip-detect", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_two_stage.json"))
    a = p.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "two_stage", "device": torch.cuda.get_device_name(0), "M": M, "num_point": P, "map": [C, HW, HW], "code_size": CODE,
           "iters": a.iters, "warmup": a.warmup, "timing": "HIP events (refine), wall clock around synchronised calls (detect); alternating",
           "baseline": "the reference's formulation in stock PyTorch-ROCm ops on the same GPU and inputs", "refine": []}
    for B in a.batches:
        res["refine"].append(bench_refine(B, a, dev))
        print(json.dumps(res["refine"][-1]))
    if not a.skip_detect:
        res["detect"] = bench_detect(a, dev)
        print(json.dumps(res["detect"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
