#!/usr/bin/env python3
"""Measure the VoxelNet detector's sparse 3-D middle (3dal_pytorch_amd/sparse.py, dal3_sp_*) on the production grid and
write profiles/bench_sparse.json:

    python tools/bench_sparse.py [--batches 1 4] [--points 180000] [--iters 20] [--warmup 5] [--out profiles/bench_sparse.json]

One sweep is `--points` seeded points per sample on the grid of configs/waymo/voxelnet (voxel 0.1 x 0.1 x 0.15 m, range
+-75.2 m / -2 .. 4 m, 41 x 1504 x 1504 sparse cells, max_points 5). Per batch size it records the active sites of every
level, the time of the bookkeeping (sort, downsample, neighbour tables) and of every level's convolutions (HIP events
around the enqueued launches, the median of `--iters` runs after `--warmup`), the executed multiply-accumulates (present
taps only, counted from the neighbour tables) and that rate over the fp32-MFMA peak, and `VoxelNet.detect` end to end
with random weights (wall clock around the call, which ends in the read-back of the kept boxes).

What this is not: there is no dense or spconv baseline on these machines (spconv is CUDA-only), so nothing here is a
speed-up; and the cloud is synthetic (rings of a spinning lidar over a flat ground with boxes of clutter), so its
occupancy is not Waymo's. No pass mark is set on any time. The capacities of the strided levels are the counts of a
first, unmeasured run with the safe bounds, plus a tenth.

    python tools/bench_sparse.py --precision fp16|bf16 [--rounds 5] [--out profiles/bench_sparse_lp.json]

measures the 16-bit route (`sparse_precision`) against the fp32 route IN THE SAME JOB on the same sweep: the bookkeeping
once (it is the same code for both), then `--rounds` rounds that alternate the two routes — every level's convolutions,
the whole backbone forward, and `VoxelNet.detect` with both knobs (`precision` and `sparse_precision`) at fp32 and at the
16-bit type. Per route it records each round's figure, their median and their spread (max - min), and whether the slowest
16-bit round beat the fastest fp32 round: the yardstick is this job's own fp32 convolutions, not another day's number."""
import argparse
import copy
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sparse = importlib.import_module("3dal_pytorch_amd.sparse")
pillars = importlib.import_module("3dal_pytorch_amd.pillars")
detector = importlib.import_module("3dal_pytorch_amd.detector")

PEAK_TFLOPS = 157.3                             # fp32 MFMA: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz
VOXEL, RANGE, MAX_POINTS, MAX_VOXELS = (0.1, 0.1, 0.15), (-75.2, -75.2, -2.0, 75.2, 75.2, 4.0), 5, 150000
STRIDED = ("conv2", "conv3", "conv4", "extra_conv")


def cloud(n, seed):
    """a spinning lidar's rings over flat ground, and clutter up to 3 m: (n, 5) float32"""
    g = np.random.default_rng(seed)
    beam = np.deg2rad(g.uniform(-17.6, 2.4, n))
    az = g.uniform(-np.pi, np.pi, n)
    r = np.minimum(1.9 / np.maximum(np.tan(-beam), 1e-3), g.uniform(3.0, 75.0, n))       # the ground, or something in front of it
    z = 1.9 - 1.9 + r * np.tan(beam) + 0.0
    xyz = np.stack([r * np.cos(az), r * np.sin(az), np.clip(z, -1.95, 3.9)], 1)
    return np.concatenate([xyz, g.uniform(0, 1, (n, 2))], 1).astype(np.float32)


def timed(fn, iters, warmup):
    out = None
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


class Walk:
    """SpMiddleResNetFHD.forward cut into its bookkeeping and its convolutions, level by level"""

    def __init__(self, model, feat, coors, B, grid, n, caps):
        self.m, self.feat, self.coors, self.B, self.n, self.caps = model, feat, coors, B, n, caps
        self.shape = (grid[2] + 1, grid[1], grid[0])
        self.packs = dict(zip(model.STEMS, model.packed()))

    def book(self, x, name):
        """the level's bookkeeping -> what its convolutions need"""
        if name == "conv_input":
            return x, sparse.subm_table(x, "res0"), None
        conv = getattr(self.m, name)[0]
        idx, keys, n_out, cap, shape = sparse.downsample(x, conv.kernel_size, conv.stride, conv.padding, self.caps.get(name))
        table = sparse.neighbour_table(x, idx, n_out, cap, shape, conv.kernel_size, conv.stride, conv.padding)
        y = sparse.SparseConvTensor(torch.empty((cap, conv.out_channels), dtype=torch.float32, device=idx.device), idx, shape, self.B,
                                    n_out, x.status)
        y.sorted = (keys, None)
        t27 = sparse.subm_table(y, "res") if name != "extra_conv" else None
        return y, t27, table

    def convs(self, x, y, t27, table, name):
        conv = getattr(self.m, name)[0]
        if name == "conv_input":
            y = x.like(sparse.conv(x.features, t27, x.n, self.packs[name], conv.in_channels, 16, x.status, relu=True, center_tap=13))
        elif name == "extra_conv":
            D, H, W = y.spatial_shape
            bev = torch.empty((self.B, 128 * D, H, W), dtype=torch.float32, device=x.features.device)
            return sparse.conv(x.features, table, y.n, self.packs[name], 128, 128, x.status, relu=True, canvas=bev,
                               out_indices=y.indices, canvas_shape=y.spatial_shape)
        else:
            f = sparse.conv(x.features, table, y.n, self.packs[name], conv.in_channels, conv.out_channels, x.status, relu=True)
            y = y.like(f)
        seq = getattr(self.m, "conv1" if name == "conv_input" else name)
        for blk in seq:
            if isinstance(blk, sparse.SparseBasicBlock):
                p1, p2 = blk.packed()
                c = blk.conv1.out_channels
                h = sparse.conv(y.features, t27, y.n, p1, c, c, y.status, relu=True, center_tap=13)
                y = y.like(sparse.conv(h, t27, y.n, p2, c, c, y.status, relu=True, residual=y.features, center_tap=13))
        return y


class WalkLp(Walk):
    """the same cut on 16-bit operands: a stem and a block's conv2 write float32 rows and their 16-bit twin, a block's conv1
    the 16-bit rows only, every layer but the first gathers 16-bit rows (SpMiddleResNetFHD.forward's route)"""

    def convs(self, x, y, t27, table, name):
        conv = getattr(self.m, name)[0]
        kw = dict(precision=self.m.sparse_precision, relu=True)
        if name == "conv_input":
            y = x.like(*sparse.conv(x.features, t27, x.n, self.packs[name], conv.in_channels, 16, x.status, center_tap=13, out16=True, **kw))
        elif name == "extra_conv":
            D, H, W = y.spatial_shape
            bev = torch.empty((self.B, 128 * D, H, W), dtype=torch.float32, device=x.indices.device)
            return sparse.conv(None, table, y.n, self.packs[name], 128, 128, x.status, canvas=bev, out_indices=y.indices,
                               canvas_shape=y.spatial_shape, features16=x.features16, **kw)
        else:
            y = y.like(*sparse.conv(None, table, y.n, self.packs[name], conv.in_channels, conv.out_channels, x.status,
                                    features16=x.features16, out16=True, **kw))
        seq = getattr(self.m, "conv1" if name == "conv_input" else name)
        for blk in seq:
            if isinstance(blk, sparse.SparseBasicBlock):
                p1, p2 = blk.packed()
                c = blk.conv1.out_channels
                _, h16 = sparse.conv(None, t27, y.n, p1, c, c, y.status, center_tap=13, features16=y.features16, out16=True, rows=False, **kw)
                y = y.like(*sparse.conv(None, t27, y.n, p2, c, c, y.status, residual=y.features, center_tap=13, features16=h16,
                                        out16=True, **kw))
        return y


def _stats(v):
    return {"rounds": [float(x) for x in v], "median": float(np.median(v)), "spread": float(max(v) - min(v))}


def _versus(f32, lp):
    """two lists of per-round figures -> both routes' statistics, the ratio of the medians, and whether every 16-bit round
    beat every fp32 round (a difference larger than the job's own run-to-run spread)"""
    return {"fp32": _stats(f32), "lp": _stats(lp), "ratio_of_medians": float(np.median(f32) / np.median(lp)),
            "lp_faster_beyond_spread": bool(max(lp) < min(f32))}


def measure_lp(B, a, dev):
    prec = a.precision
    pts = np.concatenate([cloud(a.points, 100 + b) for b in range(B)])
    off = np.arange(B + 1, dtype=np.int64) * a.points
    dpts, doff = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    grid = [int(g) for g in pillars.grid_size(VOXEL, RANGE)]
    torch.manual_seed(0)
    model = sparse.SpMiddleResNetFHD(num_input_features=5).to(dev).eval()
    model_lp = copy.deepcopy(model)
    model_lp.sparse_precision = prec
    reader = pillars.VoxelFeatureExtractorV3(num_input_features=5)
    r = pillars.voxelize(dpts, off, VOXEL, RANGE, MAX_POINTS, MAX_VOXELS, point_offsets_device=doff)
    feat = reader(r.voxels, r.num_points, n_pillars=r.n_pillars)
    with torch.no_grad():
        _, levels = model(feat, r.coordinates, B, grid, n_voxels=r.n_pillars)       # the safe bounds: counts only
        counts = {"conv1": int(r.n_pillars.item()), **{k: int(levels[k].n.item()) for k in ("conv2", "conv3", "conv4")}}
        assert int(model.last_status.item()) == 0
        del levels
        caps = {k: int(counts[k] * 1.1) + 32 for k in ("conv2", "conv3", "conv4")}
        caps["extra_conv"] = caps["conv4"]
        walks = {"fp32": Walk(model, feat, r.coordinates, B, grid, r.n_pillars, caps),
                 "lp": WalkLp(model_lp, feat, r.coordinates, B, grid, r.n_pillars, caps)}
        row = {"B": B, "points": int(pts.shape[0]), "grid": [grid[2] + 1, grid[1], grid[0]], "capacities": caps, "active_sites": counts,
               "precision": prec, "rounds": a.rounds, "levels": {}}
        # the bookkeeping, once: the same code serves both routes; its outputs are kept for the rounds
        w = walks["fp32"]
        x = sparse.SparseConvTensor(feat, r.coordinates, w.shape, B, n=r.n_pillars)
        start, books, book_ms = x, {}, {}
        for name in model.STEMS:
            def book(x=x, name=name):
                x.sorted, x.indice_dict = (None if name == "conv_input" else x.sorted), {}
                return w.book(x, name)
            book_ms[name], books[name] = timed(book, a.iters, a.warmup)
            if name != "extra_conv":
                x = w.convs(x, *books[name], name)
        row["bookkeeping_ms"] = float(sum(book_ms.values()))
        per = {k: {name: [] for name in model.STEMS} for k in walks}
        fwd = {k: [] for k in walks}
        for rnd in range(a.rounds):
            for k in ("fp32", "lp"):
                x = start
                for name in model.STEMS:
                    y, t27, table = books[name]
                    ms, out = timed(lambda: walks[k].convs(x, y, t27, table, name), a.iters, a.warmup if rnd == 0 else 1)
                    per[k][name].append(ms)
                    if name != "extra_conv":
                        x = out
                m = model if k == "fp32" else model_lp
                ms, _ = timed(lambda: m(feat, r.coordinates, B, grid, n_voxels=r.n_pillars, capacities=caps), a.iters,
                              a.warmup if rnd == 0 else 1)
                fwd[k].append(ms)
        for name in model.STEMS:
            level = "conv1" if name == "conv_input" else name
            row["levels"][level] = dict(_versus(per["fp32"][name], per["lp"][name]), bookkeeping_ms=book_ms[name])
        tot = {k: [sum(per[k][name][i] for name in model.STEMS) for i in range(a.rounds)] for k in walks}
        row["conv_ms"] = _versus(tot["fp32"], tot["lp"])
        row["backbone_forward_ms"] = _versus(fwd["fp32"], fwd["lp"])
        # the same sweep gives the same sites, and the 16-bit BEV map is the fp32 one to 16-bit accuracy
        b32 = model(feat, r.coordinates, B, grid, n_voxels=r.n_pillars, capacities=caps)[0]
        b16 = model_lp(feat, r.coordinates, B, grid, n_voxels=r.n_pillars, capacities=caps)[0]
        assert int(model_lp.last_status.item()) == 0
        row["bev_rms_difference_over_rms"] = float(((b16 - b32).double().pow(2).mean().sqrt() / b32.double().pow(2).mean().sqrt()).item())
        del b32, b16
    test_cfg = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0], nms=dict(nms_pre_max_size=4096, nms_post_max_size=500,
                    nms_iou_threshold=0.7), score_threshold=0.1, pc_range=list(RANGE[:2]), out_size_factor=8, voxel_size=list(VOXEL[:2]))
    det = detector.VoxelNet(
        reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5), backbone=model,
        neck=dict(type="RPN", layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[128, 256], us_layer_strides=[1, 2],
                  us_num_filters=[256, 256], num_input_features=256),
        bbox_head=dict(type="CenterHead", in_channels=512, tasks=[dict(num_class=3, class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"])],
                       dataset="waymo", weight=2, code_weights=[1.0] * 8,
                       common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2)}),
        test_cfg=test_cfg, max_points=MAX_POINTS, max_voxels=MAX_VOXELS, voxel_size=VOXEL, pc_range=RANGE, sparse_capacities=caps)
    det = det.to(dev).eval()
    wall = {"fp32": [], "lp": []}
    for rnd in range(a.rounds):
        for k, p in (("fp32", "fp32"), ("lp", prec)):
            det.precision = det.sparse_precision = p
            t = []
            for i in range((a.warmup if rnd == 0 else 1) + a.iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                det.detect(dpts, off, point_offsets_device=doff)
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            wall[k].append(float(np.median(t[-a.iters:])))
    row["detect_end_to_end_ms"] = _versus(wall["fp32"], wall["lp"])
    return row


def measure(B, a, dev):
    pts = np.concatenate([cloud(a.points, 100 + b) for b in range(B)])
    off = np.arange(B + 1, dtype=np.int64) * a.points
    dpts, doff = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    grid = [int(g) for g in pillars.grid_size(VOXEL, RANGE)]
    torch.manual_seed(0)
    model = sparse.SpMiddleResNetFHD(num_input_features=5).to(dev).eval()
    reader = pillars.VoxelFeatureExtractorV3(num_input_features=5)
    r = pillars.voxelize(dpts, off, VOXEL, RANGE, MAX_POINTS, MAX_VOXELS, point_offsets_device=doff)
    feat = reader(r.voxels, r.num_points, n_pillars=r.n_pillars)
    with torch.no_grad():
        _, levels = model(feat, r.coordinates, B, grid, n_voxels=r.n_pillars)       # the safe bounds: counts only
        counts = {"conv1": int(r.n_pillars.item()), **{k: int(levels[k].n.item()) for k in ("conv2", "conv3", "conv4")}}
        assert int(model.last_status.item()) == 0
        del levels
        caps = {k: int(counts[k] * 1.1) + 32 for k in ("conv2", "conv3", "conv4")}
        caps["extra_conv"] = caps["conv4"]
        w = Walk(model, feat, r.coordinates, B, grid, r.n_pillars, caps)
        row = {"B": B, "points": int(pts.shape[0]), "grid": [grid[2] + 1, grid[1], grid[0]], "capacities": caps, "levels": {}}
        x = sparse.SparseConvTensor(feat, r.coordinates, w.shape, B, n=r.n_pillars)
        total_macs = total_ms = book_ms = 0.0
        for name in model.STEMS:
            def book(x=x, name=name):
                x.sorted, x.indice_dict = (None if name == "conv_input" else x.sorted), {}
                return w.book(x, name)
            ms_b, (y, t27, table) = timed(book, a.iters, a.warmup)
            ms_c, out = timed(lambda: w.convs(x, y, t27, table, name), a.iters, a.warmup)
            n = int(y.n.item()) if y.n is not None else y.capacity
            c_in, c_out = getattr(model, name)[0].in_channels, getattr(model, name)[0].out_channels
            macs = 0
            if table is not None:
                macs += int((table[:, :n] >= 0).sum().item()) * c_in * c_out
            if t27 is not None:
                present = int((t27[:, :n] >= 0).sum().item())
                macs += present * (c_in * c_out if name == "conv_input" else 0) + 4 * present * c_out * c_out
            level = "conv1" if name == "conv_input" else name
            row["levels"][level] = {"active_sites": n, "bookkeeping_ms": ms_b, "conv_ms": ms_c, "executed_macs": macs,
                                    "executed_tflops": 2 * macs / (ms_c * 1e-3) / 1e12,
                                    "share_of_peak": 2 * macs / (ms_c * 1e-3) / 1e12 / PEAK_TFLOPS}
            total_macs, total_ms, book_ms = total_macs + macs, total_ms + ms_c, book_ms + ms_b
            if name != "extra_conv":
                x = out
        row.update(bookkeeping_ms=book_ms, conv_ms=total_ms, executed_tflop_per_sweep=2 * total_macs / 1e12 / B,
                   executed_tflops=2 * total_macs / (total_ms * 1e-3) / 1e12,
                   share_of_peak=2 * total_macs / (total_ms * 1e-3) / 1e12 / PEAK_TFLOPS)
        ms, _ = timed(lambda: model(feat, r.coordinates, B, grid, n_voxels=r.n_pillars, capacities=caps), a.iters, a.warmup)
        row["backbone_forward_ms"] = ms
    # the detector end to end, random weights: wall clock, the call ends in a read-back
    test_cfg = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0], nms=dict(nms_pre_max_size=4096, nms_post_max_size=500,
                    nms_iou_threshold=0.7), score_threshold=0.1, pc_range=list(RANGE[:2]), out_size_factor=8, voxel_size=list(VOXEL[:2]))
    det = detector.VoxelNet(
        reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5), backbone=model,
        neck=dict(type="RPN", layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[128, 256], us_layer_strides=[1, 2],
                  us_num_filters=[256, 256], num_input_features=256),
        bbox_head=dict(type="CenterHead", in_channels=512, tasks=[dict(num_class=3, class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"])],
                       dataset="waymo", weight=2, code_weights=[1.0] * 8,
                       common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2)}),
        test_cfg=test_cfg, max_points=MAX_POINTS, max_voxels=MAX_VOXELS, voxel_size=VOXEL, pc_range=RANGE, sparse_capacities=caps)
    det = det.to(dev).eval()
    wall = []
    for i in range(a.warmup + a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        det.detect(dpts, off, point_offsets_device=doff)
        torch.cuda.synchronize()
        if i >= a.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    row["detect_end_to_end_ms"] = float(np.median(wall))
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    p.add_argument("--points", type=int, default=180000)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    p.add_argument("--precision", choices=("fp16", "bf16"), default=None, help="measure this 16-bit route against fp32, alternating")
    p.add_argument("--rounds", type=int, default=5)
    a = p.parse_args()
    dev = torch.device("cuda:0")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "bench_sparse_lp.json" if a.precision else "bench_sparse.json")
    if a.precision:
        res = {"bench": "sparse_lp", "device": torch.cuda.get_device_name(0), "precision": a.precision, "voxel_size": VOXEL,
               "pc_range": RANGE, "max_points": MAX_POINTS, "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds,
               "yardstick": "this job's own fp32 route on the same sweep, alternating round by round; times in ms, HIP events "
                            "around the enqueued launches (detect: wall clock around the call, which ends in a read-back)",
               "cloud": "synthetic (seeded lidar rings over flat ground): its occupancy is not Waymo's", "rows": []}
        for B in a.batches:
            res["rows"].append(measure_lp(B, a, dev))
            print(json.dumps(res["rows"][-1]))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    res = {"bench": "sparse", "device": torch.cuda.get_device_name(0), "peak_tflops": PEAK_TFLOPS, "voxel_size": VOXEL, "pc_range": RANGE,
           "max_points": MAX_POINTS, "iters": a.iters, "warmup": a.warmup,
           "baseline": "none: spconv is CUDA-only and no dense 3-D baseline fits the production grid; nothing here is a speed-up",
           "cloud": "synthetic (seeded lidar rings over flat ground): its occupancy is not Waymo's", "rows": []}
    for B in a.batches:
        res["rows"].append(measure(B, a, dev))
        print(json.dumps(res["rows"][-1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
