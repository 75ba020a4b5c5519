#!/usr/bin/env python3
"""Measure the first stage's targets and loss (3dal_pytorch_amd/center_loss.py, rpn.CenterHead.loss: dal3_center_targets,
dal3_center_loss) and write profiles/bench_center_loss.json:

    python tools/bench_center_loss.py [--batches 1 4] [--iters 30] [--warmup 5] [--out profiles/bench_center_loss.json]

At the two real map shapes, 188 x 188 (0.1 m voxels, out_size_factor 8) and 468 x 468 (0.32 m pillars, factor 1), B in
--batches, one task of 3 classes with the five heads, max_objs 500 and 60 objects a sample: `center_targets`, `loss` +
`backward()` on maps that are autograd leaves, and `loss_from_gt` + `backward()`, beside the BASELINE for the loss: the
reference's formulation in stock PyTorch-ROCm ops on the same GPU and inputs — `_sigmoid`, FastFocalLoss, RegLoss and the
head's combination restated here, with autograd. (The reference makes the targets on the host, in its data pipeline; they
have no stock counterpart on the device.) Wall clock around synchronised calls; every shape warmed; the two alternate inside
one process; medians and spreads are recorded. No ratio is fixed in advance."""
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

rpn = importlib.import_module("3dal_pytorch_amd.rpn")
center_loss = importlib.import_module("3dal_pytorch_amd.center_loss")

SHAPES = {188: dict(range=[-75.2, -75.2, -2.0, 75.2, 75.2, 4.0], size=[0.1, 0.1, 0.15], shape=[1504, 1504, 40], out_size_factor=8),
          468: dict(range=[-74.88, -74.88, -2.0, 74.88, 74.88, 4.0], size=[0.32, 0.32, 6.0], shape=[468, 468, 1], out_size_factor=1)}
CLASSES, MAX_OBJS, OBJECTS = 3, 500, 60
CODE_WEIGHTS, WEIGHT = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0], 0.25
HEADS = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
CHANNELS = dict(hm=CLASSES, reg=2, height=1, dim=3, vel=2, rot=2)


def ground_truth(B, hw, dev, seed=3):
    """(B, 60, 10): boxes inside the range, the classes ascending as the pipeline's flattening leaves them"""
    g = torch.Generator().manual_seed(seed)
    s = SHAPES[hw]
    u = torch.rand((B, OBJECTS, 9), generator=g)
    lo, hi = s["range"][0] + 1.0, s["range"][3] - 1.0
    gt = torch.zeros((B, OBJECTS, 10))
    gt[..., 0:2] = lo + (hi - lo) * u[..., 0:2]
    gt[..., 2] = -1.0 + 2.0 * u[..., 2]
    gt[..., 3] = 0.6 + 2.0 * u[..., 3]
    gt[..., 4] = 0.8 + 4.5 * u[..., 3]
    gt[..., 5] = 1.2 + u[..., 4]
    gt[..., 6] = -3.0 + 6.0 * u[..., 5]
    gt[..., 7:9] = -4.0 + 8.0 * u[..., 6:8]
    gt[..., 9] = torch.sort(1 + (u[..., 8] * CLASSES).long(), dim=1).values.float()
    return gt.to(dev)


def at_cells(maps, ind):
    """(B, C, H, W) maps read at the flat cells ind (B, M) -> (B, M, C)"""
    flat = maps.flatten(2)
    sample = torch.arange(flat.shape[0], device=flat.device)[:, None]
    return flat[sample, :, ind]


def stock_loss(preds, ex):
    """one task of the head's loss in stock ops: the clamped sigmoid, the penalty-reduced focal loss, the masked L1 per
    column and their weighted sum"""
    p = torch.sigmoid(preds["hm"]).clamp(1e-4, 1 - 1e-4)
    ind, live = ex["ind"][0], ex["mask"][0].float()
    negatives = ((1 - p).log() * p ** 2 * (1 - ex["hm"][0]) ** 4).sum()
    peak = at_cells(p, ind).gather(2, ex["cat"][0][:, :, None])
    positives = (peak.log() * (1 - peak) ** 2 * live[:, :, None]).sum()
    count = live.sum()
    hm_loss = -(negatives if count == 0 else (positives + negatives) / count)         # the branch reads the count back
    box = torch.cat([preds[h] for h in ("reg", "height", "dim", "vel", "rot")], dim=1)
    m = live[:, :, None]
    elem = ((at_cells(box, ind) * m - ex["anno_box"][0] * m).abs() / (m.sum() + 1e-4)).sum(0).sum(0)
    loc = (elem * torch.tensor(CODE_WEIGHTS, device=elem.device)).sum()
    return hm_loss + WEIGHT * loc


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    v = np.asarray(v)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "p90_ms": float(np.percentile(v, 90)), "n": int(v.size)}


def bench(hw, B, a, dev):
    torch.manual_seed(1)
    s = SHAPES[hw]
    cfg = dict(out_size_factor=s["out_size_factor"], gaussian_overlap=0.1, max_objs=MAX_OBJS, min_radius=2,
               target_assigner=dict(tasks=[dict(num_class=CLASSES, class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"])]))
    voxels = dict(shape=np.asarray(s["shape"]), range=np.asarray(s["range"], np.float32), size=np.asarray(s["size"], np.float32))
    assigner = center_loss.AssignLabel(cfg=cfg, voxels=voxels)
    head = rpn.CenterHead(in_channels=16, tasks=cfg["target_assigner"]["tasks"], dataset="nuscenes", weight=WEIGHT,
                          code_weights=CODE_WEIGHTS, common_heads=HEADS, share_conv_channel=64).to(dev)
    gt = ground_truth(B, hw, dev)
    maps = {h: torch.randn((B, c, hw, hw), device=dev).requires_grad_(True) for h, c in CHANNELS.items()}
    maps["hm"].data.mul_(1.5).sub_(2.19)
    ex = assigner(gt)
    assert int(ex["status"].item()) == 0 and tuple(ex["hm"][0].shape) == (B, CLASSES, hw, hw)

    def zero():
        for m in maps.values():
            m.grad = None

    def targets():
        return assigner(gt)

    def fused():
        zero()
        out = head.loss(ex, [maps])["loss"][0]
        out.backward()
        return out.detach()

    def chained():
        zero()
        out = head.loss_from_gt([maps], gt, assigner)["loss"][0]
        out.backward()
        return out.detach()

    def stock():
        zero()
        out = stock_loss(maps, ex)
        out.backward()
        return out.detach()
    for _ in range(a.warmup):
        targets(), chained()
        mine, base = fused(), stock()
    torch.cuda.synchronize()
    info = {"objects_kept": int(ex["mask"][0].sum()), "loss_fused": float(mine), "loss_stock": float(base)}
    w = {k: [] for k in ("targets", "fused", "chained", "stock")}
    for _ in range(a.iters):
        for k, fn in (("targets", targets), ("fused", fused), ("stock", stock), ("chained", chained)):
            w[k].append(wall(fn)[0])
    return {"map": [hw, hw], "B": B, "center_targets": stats(w["targets"]), "loss_backward_fused": stats(w["fused"]),
            "loss_backward_stock_pytorch": stats(w["stock"]), "loss_from_gt_backward": stats(w["chained"]),
            "fused_over_stock": float(np.median(w["fused"]) / np.median(w["stock"])), "sample": info}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    p.add_argument("--maps", type=int, nargs="+", default=[188, 468], choices=sorted(SHAPES))
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_center_loss.json"))
    a = p.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "center_loss", "device": torch.cuda.get_device_name(0), "classes": CLASSES, "max_objs": MAX_OBJS, "objects": OBJECTS,
           "heads": list(CHANNELS), "iters": a.iters, "warmup": a.warmup,
           "timing": "wall clock around synchronised calls; the fused and the stock loss alternate inside one process",
           "baseline": "the reference's _sigmoid, FastFocalLoss, RegLoss and combination in stock PyTorch-ROCm ops with autograd, same GPU and inputs",
           "step": []}
    for hw in a.maps:
        for B in a.batches:
            res["step"].append(bench(hw, B, a, dev))
            print(json.dumps(res["step"][-1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
