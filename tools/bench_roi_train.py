#!/usr/bin/env python3
"""Measure the second stage's training step (3dal_pytorch_amd/two_stage.py: dal3_roi_targets, the sampled rows' gather,
the head in train mode, dal3_roi_loss, backward) and write profiles/bench_roi_train.json:

    python tools/bench_roi_train.py [--batches 1 4] [--iters 30] [--warmup 5] [--out profiles/bench_roi_train.json]

`TwoStageDetector.roi_loss(...)["loss"].backward()` at B in --batches, 500 slots a sample, ROI_PER_IMAGE 128, 60 GT rows, a
512 x 188 x 188 BEV map, 5 points a box, the production widths and code size 9, beside the BASELINE: the reference's
formulation in stock PyTorch-ROCm ops on the same GPU and inputs — the features of all 500 slots (tools/bench_two_stage.py's
indexed bilinear over a permuted copy of the map), ProposalTargetLayer as the reference writes it (a loop over samples and
classes, `iou.boxes_iou3d` standing in for its CUDA-only extension, `nonzero()`, NumPy permutations and `torch.randint` draws),
assign_targets, the Sequential stacks in train mode, the two layer losses with their `.item()` read-backs, backward. HIP
events around the enqueued work for the fused route, wall clock around synchronised calls for both (the baseline reads
back); every shape warmed; the two alternate inside one process; medians and spreads are recorded. No ratio is fixed in
advance."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_two_stage as TS  # noqa: E402

two_stage = importlib.import_module("3dal_pytorch_amd.two_stage")
iou = importlib.import_module("3dal_pytorch_amd.iou")

M, P, C, HW, CODE, ROWS, G = TS.M, TS.P, TS.C, TS.HW, TS.CODE, 128, 60
TARGET = dict(ROI_PER_IMAGE=ROWS, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75,
              CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
LOSS = dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="L1",
            LOSS_WEIGHTS={"rcnn_cls_weight": 1.0, "rcnn_reg_weight": 1.0, "code_weights": [1.0] * 7 + [0.2, 0.2]})
MODEL_CFG = dict(TS.MODEL_CFG, TARGET_CONFIG=TARGET, LOSS_CONFIG=LOSS)


def ground_truth(r, B, dev, seed=3):
    """G rows a sample: the first 50 kept boxes a little moved (fg and hard bg among the RoIs), 10 zero rows"""
    g = torch.Generator().manual_seed(seed)
    gt = torch.zeros((B, G, CODE + 1), device=dev)
    rows = r["keep"].long() + r["seg_offsets_device"][:B, None]
    for b in range(B):
        box = r["boxes"][rows[b, :50]][:, [0, 1, 2, 3, 4, 5, 8, 6, 7]].clone()
        box[:, :2] += (torch.rand((50, 2), generator=g).to(dev) - 0.5) * box[:, 3:5] * 0.6
        gt[b, :50, :CODE] = box
        gt[b, :50, CODE] = (r["labels"][rows[b, :50]] + 1).float()
    return gt


def stock_features(m, r, bev):
    """tools/bench_two_stage.py's stock route up to the padded rois and their features"""
    ext, B = m.second_stage[0], r["B"]
    rows = r["keep"].long() + r["seg_offsets_device"][:B, None]
    nhwc = bev.permute(0, 2, 3, 1).contiguous()
    rois = torch.zeros((B, M, CODE), device=bev.device)
    feats = torch.zeros((B, M, P * C), device=bev.device)
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
    return rois, r["scores"][rows], r["labels"][rows].long() + 1, feats


def stock_sample(overlaps):
    """subsample_rois / sample_bg_inds as the reference writes them"""
    fg_n = int(np.round(TARGET["FG_RATIO"] * ROWS))
    fg = (overlaps >= min(TARGET["REG_FG_THRESH"], TARGET["CLS_FG_THRESH"])).nonzero().view(-1)
    easy = (overlaps < TARGET["CLS_BG_THRESH_LO"]).nonzero().view(-1)
    hard = ((overlaps < TARGET["REG_FG_THRESH"]) & (overlaps >= TARGET["CLS_BG_THRESH_LO"])).nonzero().view(-1)

    def background(n):
        if hard.numel() and easy.numel():
            hn = min(int(n * TARGET["HARD_BG_RATIO"]), len(hard))
            return torch.cat([hard[torch.randint(0, hard.numel(), (hn,), device=hard.device)],
                              easy[torch.randint(0, easy.numel(), (n - hn,), device=easy.device)]])
        both = hard if hard.numel() else easy
        return both[torch.randint(0, both.numel(), (n,), device=both.device)]
    if fg.numel() and hard.numel() + easy.numel():
        n = min(fg_n, fg.numel())
        perm = torch.from_numpy(np.random.permutation(fg.numel())).to(fg.device).long()
        return torch.cat([fg[perm[:n]], background(ROWS - n)])
    if fg.numel():
        return fg[torch.from_numpy(np.floor(np.random.rand(ROWS) * fg.numel())).to(fg.device).long()]
    return background(ROWS)


def stock_step(m, r, bev, gt_all):
    """the reference's forward(training=True) + get_loss + backward in stock ops"""
    head, B = m.roi_head, r["B"]
    with torch.no_grad():
        rois_all, scores_all, labels_all, feats_all = stock_features(m, r, bev)
        rois, src, ious, feats = [], [], [], []
        for b in range(B):
            gt = gt_all[b]
            k = gt.shape[0] - 1
            while k > 0 and gt[k].sum() == 0:
                k -= 1
            gt = gt[:k + 1]
            gl = gt[:, -1].long()
            overlaps, asg = rois_all.new_zeros(M), labels_all.new_zeros(M)
            for cls in range(int(gl.min().item()), int(gl.max().item()) + 1):
                rm, gm = labels_all[b] == cls, gl == cls
                if rm.sum() > 0 and gm.sum() > 0:
                    v, i = torch.max(iou.boxes_iou3d(rois_all[b][rm][:, :7].contiguous(), gt[gm][:, :7].contiguous()), dim=1)
                    overlaps[rm] = v
                    asg[rm] = gm.nonzero().view(-1)[i]
            s = stock_sample(overlaps)
            rois.append(rois_all[b][s])
            src.append(gt[asg[s]])
            ious.append(overlaps[s])
            feats.append(feats_all[b][s])
        rois, g, ious, feats = torch.stack(rois), torch.stack(src), torch.stack(ious), torch.stack(feats)
        valid = ious > TARGET["REG_FG_THRESH"]
        fg_m, bg_m = ious > TARGET["CLS_FG_THRESH"], ious < TARGET["CLS_BG_THRESH"]
        lab = fg_m.float()
        mid = ~fg_m & ~bg_m
        lab[mid] = (ious[mid] - TARGET["CLS_BG_THRESH"]) / (TARGET["CLS_FG_THRESH"] - TARGET["CLS_BG_THRESH"])
        ry = rois[:, :, 6] - torch.floor(rois[:, :, 6] / (2 * np.pi) + 0.5) * (2 * np.pi)
        g[:, :, :6] = g[:, :, :6] - rois[:, :, :6]
        g[:, :, 6] = g[:, :, 6] - ry
        cs, sn, z, o = torch.cos(-ry).view(-1), torch.sin(-ry).view(-1), torch.zeros(B * ROWS, device=ry.device), torch.ones(B * ROWS, device=ry.device)
        rot = torch.stack((cs, -sn, z, sn, cs, z, z, z, o), dim=1).view(-1, 3, 3)
        flat = g.view(-1, 1, CODE + 1)
        g = torch.cat((torch.matmul(flat[:, :, 0:3], rot), flat[:, :, 3:]), dim=-1).view(B, ROWS, CODE + 1)
        g[:, :, 7:-1] = g[:, :, 7:-1] - rois[:, :, 7:]
        h = g[:, :, 6] % (2 * np.pi)
        opp = (h > np.pi * 0.5) & (h < np.pi * 1.5)
        h[opp] = (h[opp] + np.pi) % (2 * np.pi)
        h[h > np.pi] -= 2 * np.pi
        g[:, :, 6] = torch.clamp(h, min=-np.pi / 2, max=np.pi / 2)
    shared = head.shared_fc_layer(feats.reshape(-1, 1, P * C).permute(0, 2, 1).contiguous())
    cls = head.cls_layers(shared).transpose(1, 2).contiguous().squeeze(1)
    reg = head.reg_layers(shared).transpose(1, 2).contiguous().squeeze(1)
    each = F.binary_cross_entropy(torch.sigmoid(cls.view(-1)), lab.view(-1), reduction="none")
    mask = (lab.view(-1) >= 0).float()
    l_cls = (each * mask).sum() / torch.clamp(mask.sum(), min=1.0)
    fg_sum = valid.view(-1).long().sum().item()
    l_reg = F.l1_loss(reg, g[..., :CODE].reshape(-1, CODE), reduction="none") * reg.new_tensor(LOSS["LOSS_WEIGHTS"]["code_weights"])
    l_reg = (l_reg * valid.view(-1, 1).float()).sum() / max(fg_sum, 1)
    loss = l_cls + l_reg
    loss.item()
    loss.backward()
    return loss.detach()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def bench(B, a, dev):
    torch.manual_seed(1)
    np.random.seed(1)
    head = two_stage.RoIHead(P * C, MODEL_CFG, code_size=CODE)
    m = two_stage.TwoStageDetector(TS._First(), [TS.EXTRACTOR], head, M, num_point=P, freeze=True).to(dev)
    m.roi_head.train()
    bev = torch.relu(torch.randn((B, C, HW, HW), device=dev))
    r = TS.first_stage(B, dev)
    gt = ground_truth(r, B, dev)
    draws = torch.rand((B, M + ROWS), device=dev)

    def fused():
        m.zero_grad(set_to_none=True)
        out = m.roi_loss(r, bev, gt, draws)
        out["loss"].backward()
        return out

    def stock():
        m.zero_grad(set_to_none=True)
        return stock_step(m, r, bev, gt)
    for _ in range(a.warmup):
        out, base = fused(), stock()
    torch.cuda.synchronize()
    assert int(out["status"].item()) == 0
    t = out["targets"]
    info = {"fg_rows": int(t["reg_valid_mask"].sum()), "empty_rows": int((t["sample"] < 0).sum()), "loss_fused": float(out["loss"]),
            "loss_stock": float(base)}
    ev, w_fused, w_stock = [], [], []
    for _ in range(a.iters):
        ev.append(TS.event_ms(fused)[0])
        w_fused.append(wall(fused)[0])
        w_stock.append(wall(stock)[0])
    return {"B": B, "rows": B * ROWS, "fused_events": TS.stats(ev), "fused_wall": TS.stats(w_fused), "stock_pytorch_wall": TS.stats(w_stock),
            "fused_over_stock": float(np.median(w_fused) / np.median(w_stock)), "sample": info}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_roi_train.json"))
    a = p.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "roi_train", "device": torch.cuda.get_device_name(0), "M": M, "roi_per_image": ROWS, "gt_rows": G, "num_point": P,
           "map": [C, HW, HW], "code_size": CODE, "iters": a.iters, "warmup": a.warmup,
           "timing": "HIP events and wall clock around synchronised calls (roi_loss + backward), wall clock (baseline: it reads back); alternating",
           "baseline": "the reference's formulation in stock PyTorch-ROCm ops on the same GPU and inputs, iou.boxes_iou3d for its CUDA-only IoU",
           "step": []}
    for B in a.batches:
        res["step"].append(bench(B, a, dev))
        print(json.dumps(res["step"][-1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
