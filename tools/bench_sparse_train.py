#!/usr/bin/env python3
"""Measure the backward pass of the sparse 3-D middle (sparse.py's train_forward; dal3_sp_conv on the inverse tables,
dal3_sp_wgrad) on the production grid and write profiles/bench_sparse_train.json:

    python tools/bench_sparse_train.py [--batches 1 4] [--points 180000] [--iters 20] [--warmup 5] [--out profiles/bench_sparse_train.json]

The sweep, the grid and the tightened capacities are tools/bench_sparse.py's. Per batch size and level it records the time
of the level's forward convolutions (the eval-route kernel, unchanged: the yardstick), of the data gradients of the same
layers (dal3_sp_conv with the transposed packs on the inverse tables; the first layer, with 5 input channels, has none) and
of their weight gradients (dal3_sp_wgrad), HIP events around the enqueued launches, the median of `--iters` runs after
`--warmup`; the executed multiply-accumulates counted from the tables (dgrad and wgrad each execute the forward's
present-tap MACs, so the algorithmic ratio of backward to forward is 2.0) with that rate over the fp32-MFMA peak, and the
measured ratio (dgrad + wgrad) / forward. Last, `train_forward` + `backward()` of the whole backbone, BatchNorm in train
mode, wall clock between two synchronisations.

What this is not: there is no spconv baseline on these machines (spconv is CUDA-only), so nothing here is a speed-up, and
no pass mark is set on any time. The cloud is synthetic; its occupancy is not Waymo's."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_sparse as BS  # noqa: E402

sparse, pillars = BS.sparse, BS.pillars
PEAK_TFLOPS = BS.PEAK_TFLOPS


def level_layers(model, name, x, y, t27, table):
    """the convolutions of one level -> [(conv, rows of its input, rows of its output, forward table, inverse table or None)]"""
    stem = getattr(model, name)[0]
    if name == "conv_input":
        layers = [(stem, x, x, t27, None)]                  # 5 input channels: no data gradient
    else:
        inv = sparse.transposed_table(x, y.sorted[0], y.n, y.capacity, y.spatial_shape, stem.kernel_size, stem.stride, stem.padding)
        layers = [(stem, x, y, table, inv)]
    if name != "extra_conv":
        for blk in getattr(model, "conv1" if name == "conv_input" else name):
            if isinstance(blk, sparse.SparseBasicBlock):
                layers += [(blk.conv1, y, y, t27, t27), (blk.conv2, y, y, t27, t27)]
    return layers


def measure(B, a, dev):
    pts = np.concatenate([BS.cloud(a.points, 100 + b) for b in range(B)])
    off = np.arange(B + 1, dtype=np.int64) * a.points
    dpts, doff = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    grid = [int(g) for g in pillars.grid_size(BS.VOXEL, BS.RANGE)]
    torch.manual_seed(0)
    model = sparse.SpMiddleResNetFHD(num_input_features=5).to(dev).eval()
    reader = pillars.VoxelFeatureExtractorV3(num_input_features=5)
    r = pillars.voxelize(dpts, off, BS.VOXEL, BS.RANGE, BS.MAX_POINTS, BS.MAX_VOXELS, point_offsets_device=doff)
    feat = reader(r.voxels, r.num_points, n_pillars=r.n_pillars)
    with torch.no_grad():
        _, levels = model(feat, r.coordinates, B, grid, n_voxels=r.n_pillars)       # the safe bounds: counts only
        counts = {k: int(levels[k].n.item()) for k in ("conv2", "conv3", "conv4")}
        del levels
    caps = {k: int(counts[k] * 1.1) + 32 for k in counts}
    caps["extra_conv"] = caps["conv4"]
    row = {"B": B, "points": int(pts.shape[0]), "grid": [grid[2] + 1, grid[1], grid[0]], "capacities": caps, "levels": {}}
    tot = {"forward_ms": 0.0, "dgrad_ms": 0.0, "wgrad_ms": 0.0}
    with torch.no_grad():
        w = BS.Walk(model, feat, r.coordinates, B, grid, r.n_pillars, caps)
        x = sparse.SparseConvTensor(feat, r.coordinates, w.shape, B, n=r.n_pillars)
        for name in model.STEMS:
            y, t27, table = w.book(x, name)
            ms_f, out = BS.timed(lambda: w.convs(x, y, t27, table, name), a.iters, a.warmup)
            layers = level_layers(model, name, x, y, t27, table)
            jobs, macs_d, macs_w = [], 0, 0
            for conv, xin, yout, tab, inv in layers:
                n_out = yout.capacity if yout.n is None else int(yout.n.item())
                present = int((tab[:, :n_out] >= 0).sum().item())
                macs = present * conv.in_channels * conv.out_channels
                dy = torch.randn((tab.shape[1], conv.out_channels), dtype=torch.float32, device=dev)
                fin = torch.randn((xin.capacity, conv.in_channels), dtype=torch.float32, device=dev)
                pack = None
                if inv is not None:
                    wt = (conv.weight.flip(0, 1, 2) if conv.subm else conv.weight).transpose(3, 4).contiguous()
                    pack = sparse._pack_raw(wt, None, conv.kernel_size)
                    macs_d += macs
                macs_w += macs
                jobs.append((conv, xin, yout, tab, inv, dy, fin, pack))

            def dgrad():
                for conv, xin, yout, tab, inv, dy, fin, pack in jobs:
                    if inv is not None:
                        sparse.conv(dy, inv, xin.n, pack, conv.out_channels, conv.in_channels, xin.status,
                                    center_tap=13 if conv.subm else -1)

            def wgrad():
                for conv, xin, yout, tab, inv, dy, fin, pack in jobs:
                    sparse.wgrad(fin, tab, yout.n, dy, conv.kernel_size, conv.bias is not None)

            ms_d, _ = BS.timed(dgrad, a.iters, a.warmup)
            ms_w, _ = BS.timed(wgrad, a.iters, a.warmup)
            rate = lambda macs, ms: 2 * macs / (ms * 1e-3) / 1e12 if ms > 0 and macs else 0.0
            level = "conv1" if name == "conv_input" else name
            row["levels"][level] = {
                "active_sites": int(y.n.item()) if y.n is not None else y.capacity, "forward_ms": ms_f, "dgrad_ms": ms_d, "wgrad_ms": ms_w,
                "forward_macs": macs_w, "dgrad_macs": macs_d, "wgrad_macs": macs_w,
                "forward_share_of_peak": rate(macs_w, ms_f) / PEAK_TFLOPS, "dgrad_share_of_peak": rate(macs_d, ms_d) / PEAK_TFLOPS,
                "wgrad_share_of_peak": rate(macs_w, ms_w) / PEAK_TFLOPS, "backward_over_forward": (ms_d + ms_w) / ms_f,
                "algorithmic_backward_over_forward": (macs_d + macs_w) / macs_w}
            tot["forward_ms"] += ms_f
            tot["dgrad_ms"] += ms_d
            tot["wgrad_ms"] += ms_w
            del jobs
            if name != "extra_conv":
                x = out
    row.update(tot, backward_over_forward=(tot["dgrad_ms"] + tot["wgrad_ms"]) / tot["forward_ms"])
    # the whole backbone: train_forward + backward, BatchNorm in train mode
    model.train()
    wall = []
    for i in range(a.warmup + a.iters):
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bev, _ = model.train_forward(feat, r.coordinates, B, grid, n_voxels=r.n_pillars, capacities=caps)
        bev.sum().backward()
        torch.cuda.synchronize()
        if i >= a.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    row["train_forward_backward_ms"] = float(np.median(wall))
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    p.add_argument("--points", type=int, default=180000)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_sparse_train.json"))
    a = p.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "sparse_train", "device": torch.cuda.get_device_name(0), "peak_tflops": PEAK_TFLOPS, "voxel_size": BS.VOXEL,
           "pc_range": BS.RANGE, "max_points": BS.MAX_POINTS, "iters": a.iters, "warmup": a.warmup,
           "wgrad_slice": importlib.import_module("3dal_pytorch_amd._hip").SP_WGRAD_SLICE,
           "baseline": "none: spconv is CUDA-only; the yardstick is the same job's forward convolutions, nothing here is a speed-up",
           "cloud": "synthetic (seeded lidar rings over flat ground): its occupancy is not Waymo's", "rows": []}
    for B in a.batches:
        res["rows"].append(measure(B, a, dev))
        print(json.dumps(res["rows"][-1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
