#!/usr/bin/env python3
"""The PointPillars reader at the size of a Waymo batch: --frames sweeps of --points points drawn over +-75 m (a ground
plane, clusters and clutter), the 468 x 468 grid of 0.32 m pillars, 20 points per pillar, 60 000 pillars. Times, on the
current GPU (CUDA events, median of --reps after --warmup):
  voxelize   dal3_voxelize alone
  features   the fused feature kernel alone, canvas route (zero-fill included), on the voxelised batch
  reader     PillarReader.forward: voxelise -> features -> canvas, no host synchronisation in between
  before     the only route there was before: the NumPy restatement of the voxelisation on the host (tests/pillars_ref.py;
             on --host_frames frames, scaled to the batch), the upload of the collated batch, and the reference-formulation
             torch modules (the composite + a per-sample scatter loop) on the same GPU
and checks the reader's canvas against voxelise -> module -> scatter. The reader's bytes moved (voxels, num_points,
coordinates in; the canvas zero-filled and the pillars' cells written) are set against the HBM bandwidth figure, and the
compiler's register / scratch / LDS counts of every kernel are recorded (`kernel_resources`). One JSON line; --out writes it to a file.
    python tools/bench_pillars.py [--frames 4 --points 180000 --reps 5 --out profiles/bench_pillars.json]
"""
import argparse
import importlib
import json
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pillars = importlib.import_module("3dal_pytorch_amd.pillars")
import pillars_ref as R  # noqa: E402

CFG = dict(voxel_size=(0.32, 0.32, 6.0), pc_range=(-74.88, -74.88, -2.0, 74.88, 74.88, 4.0), max_points=20, max_voxels=60000,
           num_input_features=5, num_filters=(64, 64), norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01))
HBM_TBPS = 8.0                                  # MI355X HBM3E peak (spec); a float4 copy measures 6.29 TB/s, 79 % of it


def sweep(seed, n):
    """a lidar-like frame: 60 % ground within 75 m (density falling with range), 30 % in 40 clusters, 10 % clutter"""
    rng = np.random.default_rng(seed)
    g, c = int(0.6 * n), int(0.3 * n)
    r = 75.0 * rng.uniform(0, 1, g) ** 1.5
    th = rng.uniform(0, 2 * np.pi, g)
    ground = np.stack([r * np.cos(th), r * np.sin(th), rng.normal(-1.6, 0.05, g)], 1)
    centres = rng.uniform(-60, 60, (40, 2))
    k = rng.integers(0, 40, c)
    clusters = np.concatenate([centres[k] + rng.normal(0, 0.8, (c, 2)), rng.uniform(-1.5, 1.0, (c, 1))], 1)
    clutter = rng.uniform([-80, -80, -3], [80, 80, 5], (n - g - c, 3))
    xyz = np.concatenate([ground, clusters, clutter])[rng.permutation(n)]
    return np.concatenate([xyz, rng.uniform(0, 1, (n, 2))], 1).astype(np.float32)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), [round(t, 3) for t in ts]


def scatter_per_sample(feats, coords, B, ny, nx):
    """the scatter there was before: one masked gather and one column copy per sample, a Python loop over the batch"""
    canvas = feats.new_zeros((B, feats.shape[1], ny * nx))
    for b in range(B):
        rows = torch.nonzero(coords[:, 0] == b).squeeze(1)
        cell = coords[rows, 2].long() * nx + coords[rows, 3].long()
        canvas[b].index_copy_(1, cell, feats[rows].t().contiguous())
    return canvas.reshape(B, feats.shape[1], ny, nx)


def kernel_resources():
    """registers, scratch and LDS of every kernel of csrc/dal3_pillars.hip, from the compiler's own remarks (the library's
    flags, nothing is linked or kept) -> {kernel: {...}}, or None where there is no hipcc"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(ROOT, "3dal_pytorch_amd", "csrc", "dal3_pillars.hip")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c", src, "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    try:
        text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    except (OSError, subprocess.TimeoutExpired):
        return None
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "SGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            m2 = re.search(r"\d+([a-z_]+_kernel)(ILi(\d)ELi(\d)E)?", name)
            cur = (m2.group(1) + (f"<{m2.group(3)},{m2.group(4)}>" if m2.group(2) else "")) if m2 else name
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]+\])?): (\d+)", line)
        if m and cur and m.group(1).strip() in keys:
            out[cur][keys[m.group(1).strip()]] = int(m.group(2))
    return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--points", type=int, default=180000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host_frames", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, n = a.frames, a.points
    pts = np.concatenate([sweep(100 + b, n) for b in range(B)])
    off = np.arange(B + 1, dtype=np.int64) * n
    dev = torch.device("cuda")
    reader = pillars.PillarReader(CFG)
    reader.reader.load_state_dict({k: torch.as_tensor(v) for k, v in R.reader_weights(2, 5).items()}, strict=True)
    reader = reader.to(dev).eval()
    net = reader.reader
    grid = reader.grid
    nx, ny = int(grid[0]), int(grid[1])
    pts_dev = torch.from_numpy(pts).to(dev)
    off_dev = torch.from_numpy(off).to(dev)

    def vox():
        return pillars.voxelize(pts_dev, off, CFG["voxel_size"], CFG["pc_range"], 20, 60000, point_offsets_device=off_dev)

    r = vox()
    voxels, coords, num, nv = r.finish()
    M = int(voxels.shape[0])
    t_vox = timed(vox, a.reps, a.warmup)
    t_feat = timed(lambda: net.forward_canvas(r.voxels, r.num_points, r.coordinates, B, [nx, ny], n_pillars=r.n_pillars), a.reps,
                   a.warmup)
    t_reader = timed(lambda: reader(pts_dev, off), a.reps, a.warmup)
    canvas = reader(pts_dev, off)
    two_step = pillars.PointPillarsScatter(64)(net(voxels, num, coords), coords, B, [nx, ny])
    same = bool(torch.equal(canvas, two_step))
    # ---- the route there was before
    t0 = time.perf_counter()
    hv = [R.voxelize(pts[off[b]:off[b + 1]], CFG["voxel_size"], CFG["pc_range"], 20, 60000) for b in range(a.host_frames)]
    host_ms = (time.perf_counter() - t0) * 1e3 * B / a.host_frames
    exact = all(np.array_equal(hv[b][0].view(np.uint32), voxels[int(r.voxel_offsets[b]):int(r.voxel_offsets[b + 1])].cpu().numpy().view(np.uint32))
                for b in range(a.host_frames))
    hvox, hco, hnum = voxels.cpu(), coords.cpu(), num.cpu()
    t_upload = timed(lambda: (hvox.to(dev), hco.to(dev), hnum.to(dev)), a.reps, a.warmup)
    t_modules = timed(lambda: scatter_per_sample(net.composite(voxels, num, coords), coords, B, ny, nx), a.reps, a.warmup)
    before = scatter_per_sample(net.composite(voxels, num, coords), coords, B, ny, nx)
    bytes_moved = M * (20 * 5 * 4 + 4 + 16) + B * 64 * ny * nx * 4 + M * 64 * 4
    res = {"bench": "pillars", "frames": B, "points_per_frame": n, "grid": [nx, ny], "pillars": M,
           "pillars_per_frame": [int(v) for v in nv.cpu()], "voxelize_ms": t_vox[0], "voxelize_all": t_vox[1],
           "features_canvas_ms": t_feat[0], "features_canvas_all": t_feat[1], "reader_ms": t_reader[0], "reader_all": t_reader[1],
           "reader_equals_two_step": same, "voxels_equal_host_restatement": bool(exact),
           "before_host_voxelize_ms": host_ms, "before_upload_ms": t_upload[0], "before_torch_modules_ms": t_modules[0],
           "before_total_ms": host_ms + t_upload[0] + t_modules[0],
           "max_abs_diff_vs_torch_modules": float((canvas - before).abs().max()),
           "features_bytes_moved": bytes_moved, "features_gbps": bytes_moved / (t_feat[0] * 1e-3) / 1e9,
           "features_fraction_of_hbm_peak": bytes_moved / (t_feat[0] * 1e-3) / (HBM_TBPS * 1e12),
           "device": torch.cuda.get_device_name(0), "kernel_resources": kernel_resources()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
