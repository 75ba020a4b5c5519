#!/usr/bin/env python3
"""The pillar reader's training step at tools/bench_pillars.py's own shape: its seeded 180 k-point sweeps on the 468 x 468
grid of 0.32 m pillars, 20 points per pillar, the two-layer net, B = 1 and 4. Timed, on the current GPU:
  reader     PillarFeatureNet.train_forward_canvas + backward() under a seeded canvas cotangent (capacity-sized inputs
             with the device count), against the composite + an index_put scatter + stock autograd fed the live rows,
             sliced outside the timed region
  detector   PointPillars.first_stage_loss + backward(), reader="hip" (capacity-sized example) against reader="composite"
             (live-sliced example, prepared outside the timed region); and train_step_from_sweeps + backward() with
             reader="hip" from the resident sweeps (augmentation, voxelisation and targets included; the composite has
             no such route)
The two routes alternate for --rounds rounds in one process; a figure is wall clock around synchronised calls, reported
as the median with the fastest and the slowest round. torch.cuda.max_memory_allocated is taken per route over a round of
its own. One JSON line; --out writes it to a file.
    python tools/bench_pillars_train.py [--rounds 7 --out profiles/bench_pillars_train.json]
"""
import argparse
import functools
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pillars = importlib.import_module("3dal_pytorch_amd.pillars")
detector = importlib.import_module("3dal_pytorch_amd.detector")
augment = importlib.import_module("3dal_pytorch_amd.augment")
center_loss = importlib.import_module("3dal_pytorch_amd.center_loss")
import bench_pillars as BP  # noqa: E402
import rpn_ref  # noqa: E402

CFG = BP.CFG
CLASSES = ["VEHICLE", "PEDESTRIAN", "CYCLIST"]


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(routes, rounds, warmup=2):
    """{name: fn} -> {name: {median_ms, min_ms, max_ms, rounds_ms, peak_bytes}}: the routes take turns within a round"""
    for _ in range(warmup):
        for fn in routes.values():
            wall(fn)
    ts = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            ts[k].append(wall(fn))
    out = {}
    for k, fn in routes.items():
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        wall(fn)
        out[k] = dict(median_ms=float(np.median(ts[k])), min_ms=min(ts[k]), max_ms=max(ts[k]), rounds_ms=[round(t, 3) for t in ts[k]],
                      peak_bytes_above_resident=int(torch.cuda.max_memory_allocated() - base))
    return out


def reader_net():
    torch.manual_seed(0)
    return pillars.PillarFeatureNet(num_input_features=5, num_filters=CFG["num_filters"], voxel_size=CFG["voxel_size"],
                                    pc_range=CFG["pc_range"], norm_cfg=CFG["norm_cfg"]).cuda().train()


def model():
    torch.manual_seed(0)
    m = detector.PointPillars(
        reader=dict(type="PillarFeatureNet", num_filters=list(CFG["num_filters"]), num_input_features=5, with_distance=False,
                    voxel_size=CFG["voxel_size"], pc_range=CFG["pc_range"], norm_cfg=CFG["norm_cfg"]),
        backbone=dict(type="PointPillarsScatter", ds_factor=1), neck=dict(type="RPN", **rpn_ref.NECK),
        bbox_head=dict(type="CenterHead", **rpn_ref.HEAD), max_points=CFG["max_points"], max_voxels=CFG["max_voxels"])
    return m.cuda().train()


def boxes(B, n=24, cols=10):
    rng = np.random.default_rng(11)
    gt = np.zeros((B, 32, cols), np.float32)
    gt[:, :n, :2] = rng.uniform(-60, 60, (B, n, 2))
    gt[:, :n, 3:6] = [1.9, 4.5, 1.7]
    gt[:, :n, 6 if cols == 10 else 8] = rng.uniform(-3, 3, (B, n))
    cls = np.zeros((B, 32), np.int32)
    cls[:, :n] = rng.integers(1, 4, (B, n))
    if cols == 10:
        gt[:, :, 9] = cls
    return gt, cls


def bench(B, points, rounds):
    pts = np.concatenate([BP.sweep(100 + b, points) for b in range(B)])
    off = np.arange(B + 1, dtype=np.int64) * points
    dpts = torch.from_numpy(pts).cuda()
    grid = pillars.grid_size(CFG["voxel_size"], CFG["pc_range"])
    shape = [int(grid[0]), int(grid[1])]
    r = pillars.voxelize(dpts, off, CFG["voxel_size"], CFG["pc_range"], CFG["max_points"], CFG["max_voxels"])
    voxels, coords, num, nv = r.finish()
    live, cap = int(voxels.shape[0]), int(r.voxels.shape[0])
    voxels, coords, num = voxels.contiguous(), coords.contiguous(), num.contiguous()
    at = coords.long()
    gen = torch.Generator(device="cuda").manual_seed(3)
    cot = torch.randn((B, 64, shape[1], shape[0]), device="cuda", generator=gen)
    res = dict(B=B, points_per_frame=points, live_pillars=live, capacity=cap)
    # ---- the reader alone
    net_h, net_c = reader_net(), reader_net()

    def hip():
        for p in net_h.parameters():
            p.grad = None
        net_h.train_forward_canvas(r.voxels, r.num_points, r.coordinates, B, shape, n_pillars=r.n_pillars).backward(cot)

    def composite():
        for p in net_c.parameters():
            p.grad = None
        feats = net_c.composite(voxels, num, coords)
        canvas = feats.new_zeros((B, 64, shape[1], shape[0]))
        canvas[at[:, 0], :, at[:, 2], at[:, 3]] = feats
        canvas.backward(cot)
    res["reader"] = alternate({"hip": hip, "composite": composite}, rounds)
    worst = max(float((a.grad - b.grad).abs().max() / b.grad.abs().max()) for a, b in zip(net_h.parameters(), net_c.parameters()))
    res["reader"]["grad_max_rel_diff_hip_vs_composite"] = worst
    del net_h, net_c
    # ---- the detector
    gt10, _ = boxes(B)
    targets = center_loss.center_targets(torch.from_numpy(gt10).cuda(), [3], CFG["pc_range"], CFG["voxel_size"], 1, (shape[1], shape[0]))
    ex_live = dict(voxels=voxels, coordinates=coords, num_points=num, num_voxels=nv, shape=[shape + [1]] * B, **targets)
    ex_cap = dict(ex_live, voxels=r.voxels, coordinates=r.coordinates, num_points=r.num_points, n_voxels=r.n_pillars)
    m = model()

    def loss_step(example, reader):
        def run():
            for p in m.parameters():
                p.grad = None
            sum(m.first_stage_loss(example, reader=reader)["loss"]).backward()
        return run
    res["first_stage_loss"] = alternate({"hip": loss_step(ex_cap, "hip"), "composite": loss_step(ex_live, "composite")}, rounds)
    gen2 = torch.Generator(device="cuda").manual_seed(5)
    pre = augment.Preprocess(dict(mode="train", shuffle_points=True, global_rot_noise=0.2, global_scale_noise=[0.95, 1.05],
                                  global_translate_std=0.1, class_names=CLASSES, db_sampler=None),
                             pc_range=CFG["pc_range"], max_objs=64, generator=gen2)
    acfg = dict(out_size_factor=1, target_assigner=dict(tasks=[dict(num_class=3, class_names=CLASSES)]), gaussian_overlap=0.1,
                max_objs=64, min_radius=2)
    m.set_train_input(pre, center_loss.AssignLabel(cfg=acfg))
    gt9, cls = boxes(B, cols=9)
    ann = dict(gt_boxes=torch.from_numpy(gt9).cuda(), gt_classes=cls, gt_counts=np.full(B, 24, np.int32))

    def from_sweeps():
        for p in m.parameters():
            p.grad = None
        sum(m.train_step_from_sweeps(dpts, off, ann, reader="hip")["loss"]).backward()
    res["train_step_from_sweeps"] = alternate({"hip": from_sweeps}, rounds)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--points", type=int, default=180000)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out")
    a = ap.parse_args()
    out = dict(tool="bench_pillars_train", device=torch.cuda.get_device_name(0), rounds=a.rounds, method="wall clock around "
               "torch.cuda.synchronize, the routes alternating within a round; median, fastest and slowest round",
               runs=[bench(B, a.points, a.rounds) for B in a.batches])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
