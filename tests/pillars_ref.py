"""NumPy restatements of the PointPillars reader (3dal_pytorch_amd/pillars.py; dal3_voxelize / dal3_pillar_features /
dal3_voxel_mean of include/dal3.h), and the seeded inputs of tests/golden/pillars.npz (written by tests/golden/gen_pillars.py
from the reference's own points_to_voxel, PillarFeatureNet, PointPillarsScatter and VoxelFeatureExtractorV3).

`voxelize` is the PARALLEL formulation the kernels use — a stable sort by cell, run heads, ranks of the heads in point order
— not the reference's loop: that it equals the loop's recorded output bit for bit, cap included, is what
tests/test_pillars_cpu.py pins. `reader_f64` is the float64 truth of the feature net, `judge` the measures the GPU test
holds against the torch-CPU fp32 module's own error."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
synth = importlib.import_module("3dal_pytorch_amd.synth")

SEED = 20240611
# the pillar grid: 32 x 32 x 1 cells of 0.32 m; x and y start at different places so that swapped offsets show
PILLAR = dict(voxel_size=(0.32, 0.32, 4.0), pc_range=(0.0, -5.12, -3.0, 10.24, 5.12, 1.0), max_points=20, C=5)
PILLAR_CAPS = {"free": 2000, "cap600": 600, "cap1": 1}
# the VoxelNet-style grid: 16 x 16 x 4 cells
VOXELNET = dict(voxel_size=(0.5, 0.5, 1.0), pc_range=(-4.0, -4.0, -2.0, 4.0, 4.0, 2.0), max_points=5, max_voxels=400)
VOXELNET_CASES = {"vn_c3_rev": (3, True), "vn_c3_fwd": (3, False), "vn_c8_rev": (8, True), "vn_c8_fwd": (8, False)}
BATCH_COUNTS = (4000, 0, 500, 1777)             # sample 1 is empty, every point of sample 2 is out of range
BATCH_CAP = 320
EPS = 1e-3                                      # the reader's norm_cfg
FLOOR = 1e-30


def grid_of(voxel_size, pc_range):
    r = np.asarray(pc_range, np.float32)
    return np.round((r[3:] - r[:3]) / np.asarray(voxel_size, np.float32)).astype(np.int64)


def _ulp(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf))


def planted(cfg, C, with_nan):
    """points on each of the six faces of the range and one float32 ulp either side, on an interior cell face and one ulp
    either side, a +Inf and a -Inf point and (with_nan) a NaN point; the other coordinates sit mid-cell"""
    lo, hi = np.asarray(cfg["pc_range"][:3], np.float32), np.asarray(cfg["pc_range"][3:], np.float32)
    vs = np.asarray(cfg["voxel_size"], np.float32)
    mid = np.minimum(lo + vs * np.float32(2.5), lo + (hi - lo) * np.float32(0.5))
    rows = []
    for j in range(3):
        faces = [lo[j], hi[j]]
        if grid_of(cfg["voxel_size"], cfg["pc_range"])[j] > 1:
            faces.append(np.float32(lo[j] + vs[j] * np.float32(3)))
        for f in faces:
            for v in (_ulp(f, False), np.float32(f), _ulp(f, True)):
                p = mid.copy()
                p[j] = v
                rows.append(p)
    for bad in (np.inf, -np.inf) + ((np.nan,) if with_nan else ()):
        for j in range(3):
            p = mid.copy()
            p[j] = bad
            rows.append(p)
    xyz = np.asarray(rows, np.float32)
    out = np.zeros((xyz.shape[0], C), np.float32)
    out[:, :3] = xyz
    return out


def cloud(tag, n, cfg, C, with_nan=True, outside=False):
    """n seeded points: two thirds uniform over a box twice as wide as the range in x and y (a tenth wider in z), a third
    in a tight cluster so that pillars beyond max_points occur; with n large enough the planted points replace some of
    them. Column 3 (when there is one) is the point's index / n, which keeps every row unique. outside: every point is
    pushed beyond the upper x face."""
    lo, hi = np.asarray(cfg["pc_range"][:3], np.float64), np.asarray(cfg["pc_range"][3:], np.float64)
    pad = np.array([0.5, 0.5, 0.05]) * (hi - lo)
    pts = synth.uniform(SEED, "pillars/" + tag, (n, C), 0.0, 1.0)
    pts[:, :3] = (lo - pad) + pts[:, :3] * (hi - lo + 2 * pad)
    k = n // 3
    centre = lo + (hi - lo) * np.array([0.31, 0.62, 0.5])
    pts[:k, :3] = centre + synth.normal(SEED, "pillars/cluster/" + tag, (k, 3), 0.0, 1.0) * np.array([1.2, 1.2, 0.2]) * \
        np.asarray(cfg["voxel_size"], np.float64)
    pts = pts.astype(np.float32)
    if outside:
        pts[:, 0] = np.float32(hi[0]) + np.float32(0.5) + np.abs(pts[:, 0])
    else:
        pl = planted(cfg, C, with_nan)
        if n >= 4 * pl.shape[0]:
            at = (synth.uniform(SEED, "pillars/at/" + tag, (pl.shape[0],)) * n).astype(np.int64)
            at = np.unique(at)
            pts[at, :3] = pl[:at.size, :3]
            if at.size < pl.shape[0]:               # a collision of positions: the rest go to the end
                pts[n - (pl.shape[0] - at.size):, :3] = pl[at.size:, :3]
    if C > 3:
        pts[:, 3] = (np.arange(n, dtype=np.float64) / n).astype(np.float32)
    return pts


def drop_nan(points):
    """the reference's input: the NaN points left out (a NaN cast to an index is undefined there)"""
    return points[~np.isnan(points[:, :3]).any(1)]


def cells(points, voxel_size, pc_range):
    """-> (in range (N) bool, cell (N, 3) int64 [x, y, z]) by the definition: float32 subtraction, division, floor"""
    lo = np.asarray(pc_range, np.float32)[:3]
    vs = np.asarray(voxel_size, np.float32)
    grid = grid_of(voxel_size, pc_range)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((points[:, :3].astype(np.float32) - lo) / vs)
        ok = np.all((c >= 0) & (c < grid.astype(np.float32)), axis=1)       # a NaN fails
    return ok, np.where(ok[:, None], c, 0).astype(np.int64)


def voxelize_index(points, voxel_size, pc_range, max_points, max_voxels):
    """-> (index (M, max_points) int64: the point at each row, -1 behind the last; cell (M, 3) [x, y, z]; count (M))"""
    grid = grid_of(voxel_size, pc_range)
    ok, c = cells(points, voxel_size, pc_range)
    idx = np.nonzero(ok)[0]
    key = (c[idx, 2] * grid[1] + c[idx, 1]) * grid[0] + c[idx, 0]
    order = np.argsort(key, kind="stable")          # a cell's points together, by ascending index
    skey, spos = key[order], idx[order]
    n = skey.size
    head = np.ones(n, bool)
    head[1:] = skey[1:] != skey[:-1]
    start = np.maximum.accumulate(np.where(head, np.arange(n), 0)) if n else np.zeros(0, np.int64)
    row = np.arange(n) - start
    # the voxel index: the exclusive scan of the head flags IN POINT ORDER
    flag = np.zeros(points.shape[0], np.int64)
    flag[spos[head]] = 1
    rank = np.cumsum(flag) - flag
    vox = rank[spos[start]] if n else np.zeros(0, np.int64)
    M = min(int(flag.sum()), int(max_voxels))
    index = -np.ones((M, max_points), np.int64)
    keep = (vox < max_voxels) & (row < max_points)
    index[vox[keep], row[keep]] = spos[keep]
    cell = np.zeros((M, 3), np.int64)
    hk = head & (vox < max_voxels)
    cell[vox[hk]] = c[spos[hk]]
    count = np.zeros(M, np.int64)
    np.add.at(count, vox[vox < max_voxels], 1)
    return index, cell, np.minimum(count, max_points)


def gather(points, index):
    """the voxels of an index map: (M, max_points, C), zeros at -1"""
    out = points[np.maximum(index, 0)]
    out[index < 0] = 0
    return out


def voxelize(points, voxel_size, pc_range, max_points, max_voxels, reverse_index=True):
    """points_to_voxel's three arrays"""
    index, cell, count = voxelize_index(points, voxel_size, pc_range, max_points, max_voxels)
    coords = cell[:, ::-1] if reverse_index else cell
    return gather(points, index), coords.astype(np.int32), count.astype(np.int32)


def voxelize_batch(points, offsets, voxel_size, pc_range, max_points, max_voxels, reverse_index=True):
    """the collated batch: voxels, coordinates (M, 4) with the batch column in front, num_points, num_voxels (B)"""
    vs, cs, ns, nv = [], [], [], []
    for b in range(len(offsets) - 1):
        v, c, n = voxelize(points[offsets[b]:offsets[b + 1]], voxel_size, pc_range, max_points, max_voxels, reverse_index)
        vs.append(v)
        cs.append(np.concatenate([np.full((c.shape[0], 1), b, np.int32), c], 1))
        ns.append(n)
        nv.append(v.shape[0])
    C = points.shape[1]
    return (np.concatenate(vs) if vs else np.zeros((0, max_points, C), np.float32),
            np.concatenate(cs) if cs else np.zeros((0, 4), np.int32),
            np.concatenate(ns) if ns else np.zeros(0, np.int32), np.asarray(nv, np.int64))


def batch_points():
    """the ragged batch of the fixture: (points (sum, 5), offsets)"""
    parts = [cloud(f"batch{b}", n, PILLAR, PILLAR["C"], with_nan=True, outside=(b == 2)) for b, n in enumerate(BATCH_COUNTS)]
    off = np.concatenate([[0], np.cumsum(BATCH_COUNTS)]).astype(np.int64)
    return np.concatenate(parts), off


# ------------------------------------------------------------------------------------- the reader
def reader_weights(n_layers, C, tag="pfn"):
    """a reference-keyed state_dict of a PillarFeatureNet with num_filters (64,) * n_layers: hash weights, BatchNorm
    statistics away from (0, 1) so that the folding is exercised"""
    sd = {}
    dims = [(C + 5, 64)] if n_layers == 1 else [(C + 5, 32), (64, 64)]
    for i, (cin, cout) in enumerate(dims):
        p = f"pfn_layers.{i}."
        sd[p + "linear.weight"] = synth.normal(SEED, f"{tag}{n_layers}/{i}/w", (cout, cin), 0.0, 1.0 / np.sqrt(cin)).astype(np.float32)
        sd[p + "norm.weight"] = synth.uniform(SEED, f"{tag}{n_layers}/{i}/g", (cout,), 0.5, 1.5).astype(np.float32)
        sd[p + "norm.bias"] = synth.normal(SEED, f"{tag}{n_layers}/{i}/b", (cout,), 0.0, 0.3).astype(np.float32)
        sd[p + "norm.running_mean"] = synth.normal(SEED, f"{tag}{n_layers}/{i}/m", (cout,), 0.0, 0.5).astype(np.float32)
        sd[p + "norm.running_var"] = synth.uniform(SEED, f"{tag}{n_layers}/{i}/v", (cout,), 0.002, 2.0).astype(np.float32)
        sd[p + "norm.num_batches_tracked"] = np.asarray(7, np.int64)
    return sd


def reader_f64(sd, voxels, num_points, coords, voxel_size, pc_range, eps=EPS, fault=None):
    """PillarFeatureNet.forward (eval mode, with_distance=False) in float64 -> (P, C_out). fault: one of FAULTS"""
    n_layers = sum(1 for k in sd if k.endswith("linear.weight"))
    x = voxels.astype(np.float64)
    P, T, C = x.shape
    num = num_points.astype(np.float64)
    vx, vy = float(voxel_size[0]), float(voxel_size[1])
    xo, yo = vx / 2 + float(pc_range[0]), vy / 2 + float(pc_range[1])
    if fault == "offsets_swapped":
        xo, yo = yo, xo
    mean = x[:, :, :3].sum(1, keepdims=True) / (float(T) if fault == "mean_by_max_points" else num.reshape(-1, 1, 1))
    fc = np.stack([x[:, :, 0] - (coords[:, 3].astype(np.float64)[:, None] * vx + xo),
                   x[:, :, 1] - (coords[:, 2].astype(np.float64)[:, None] * vy + yo)], -1)
    f = np.concatenate([x, x[:, :, :3] - mean, fc], -1)
    real = np.arange(T)[None, :] < num_points[:, None]
    f = f * real[:, :, None]
    if fault == "eps_1e-5":
        eps = 1e-5
    for i in range(n_layers):
        p = f"pfn_layers.{i}."
        w = sd[p + "linear.weight"].astype(np.float64)
        y = f @ w.T
        y = (y - sd[p + "norm.running_mean"].astype(np.float64)) / np.sqrt(sd[p + "norm.running_var"].astype(np.float64) + eps)
        y = np.maximum(y * sd[p + "norm.weight"].astype(np.float64) + sd[p + "norm.bias"].astype(np.float64), 0.0)
        if fault == "padding_out_of_max":
            ymax = np.where(real[:, :, None], y, -np.inf).max(1, keepdims=True)
        else:
            ymax = y.max(1, keepdims=True)
        f = ymax if i == n_layers - 1 else np.concatenate([y, np.repeat(ymax, T, 1)], -1)
    return f.reshape(P, -1)


# The GPU test's bars: multiples of the yardstick (the torch-CPU fp32 module's own error against the float64 truth on the
# same rows). The rule: the worst ratio recorded in profiles/pillars_measured.json (DAL3_PILLARS_RECORD, tests/
# test_gpu_pillars.py) x at most 2, rounded up to one significant digit, and under a tenth of the smallest planted-fault
# ratio of tests/test_pillars_cpu.py (3.4e3). No MI355X run was to be had when they were first set, so they stand on
# reasoning: kernel and yardstick are fp32 evaluations of the same chain of <= 64-term dot products; the kernel rounds
# every folded weight once more (the rms error of a term grows by at most sqrt(2)) and sums in another order (the same
# bound), and the per-channel measures are maxima over 64 channels of a few hundred rows, which move by about 2x between
# two equally good evaluations: 4 = sqrt(2) x 2, rounded up to one significant digit.
BARS = {"tensor": 4.0, "chan_rms": 4.0, "chan_max": 4.0}
FAULTS = ("padding_out_of_max", "eps_1e-5", "mean_by_max_points", "offsets_swapped")
MEASURES = ("tensor", "chan_rms", "chan_max")


def mean_f64(voxels, num_points):
    return voxels.astype(np.float64).sum(1) / num_points.astype(np.float64)[:, None]


def judge(got, truth):
    """-> {tensor: max |d| / max |truth|; chan_rms / chan_max: the largest over channels of rms(d_c) / max|d_c| over the
    channel's own max |truth_c|; dead_ok: channels that are 0 in the truth are +0 in got}. (P, C) arrays."""
    got, truth = np.asarray(got), np.asarray(truth, np.float64)
    d = got.astype(np.float64) - truth
    scale = np.abs(truth).max(0) if truth.shape[0] else np.zeros(truth.shape[1])
    live = scale > 0
    dead_ok = bool(np.all(got[:, ~live] == 0) and not np.signbit(got[:, ~live]).any())
    if not truth.size or not live.any():
        return {"tensor": 0.0, "chan_rms": 0.0, "chan_max": 0.0, "dead_ok": dead_ok}
    return {"tensor": float(np.abs(d).max() / np.abs(truth).max()),
            "chan_rms": float((np.sqrt((d[:, live] ** 2).mean(0)) / scale[live]).max()),
            "chan_max": float((np.abs(d[:, live]).max(0) / scale[live]).max()), "dead_ok": dead_ok}


def ratios(got, f32, truth):
    """each measure of got over the same measure of the torch-CPU fp32 module (the yardstick) -> (ratios, measured, yard)"""
    m, y = judge(got, truth), judge(f32, truth)
    return {k: m[k] / max(y[k], FLOOR) for k in MEASURES}, m, y


def scatter(features, coords, batch_size, ny, nx):
    """PointPillarsScatter"""
    canvas = np.zeros((batch_size, features.shape[1], ny, nx), features.dtype)
    canvas[coords[:, 0], :, coords[:, 2], coords[:, 3]] = features
    return canvas
