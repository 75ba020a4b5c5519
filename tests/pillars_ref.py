"""NumPy restatements of the PointPillars reader (3dal_pytorch_amd/pillars.py; dal3_voxelize / dal3_pillar_features /
dal3_voxel_mean of include/dal3.h), and the seeded inputs of tests/golden/pillars.npz (written by tests/golden/gen_pillars.py
from the reference's own points_to_voxel, PillarFeatureNet, PointPillarsScatter and VoxelFeatureExtractorV3).

`voxelize` is the PARALLEL formulation the kernels use — a stable sort by cell, run heads, ranks of the heads in point order
— not the reference's loop: that it equals the loop's recorded output bit for bit, cap included, is what
tests/test_pillars_cpu.py pins. `voxelize_loop` is that loop itself, written from the definition of include/dal3.h and
pinned to the same recorded output: the oracle of the cases no fixture holds (the tables of tests/
test_gpu_pillars_edges.py, kept here so that the CPU suite walks them too). `reader_f64` is the float64 truth of the
feature net, `judge` the measures the GPU test holds against the torch-CPU fp32 module's own error."""
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


def voxelize_loop(points, voxel_size, pc_range, max_points, max_voxels):
    """the definition of include/dal3.h as the sequential loop it is stated as: walk the points in order, a dict from
    cell to voxel index assigned by first appearance, a new cell is dropped once max_voxels voxels exist, a point is
    appended while its voxel has fewer than max_points rows. No dense grid. -> voxelize_index's triple"""
    ok, c = cells(points, voxel_size, pc_range)
    voxel_of, rows, cell = {}, [], []
    for i in np.nonzero(ok)[0].tolist():
        key = (int(c[i, 0]), int(c[i, 1]), int(c[i, 2]))
        v = voxel_of.get(key)
        if v is None:
            if len(rows) >= max_voxels:
                continue
            v = voxel_of[key] = len(rows)
            rows.append([])
            cell.append(key)
        if len(rows[v]) < max_points:
            rows[v].append(i)
    index = -np.ones((len(rows), max_points), np.int64)
    for v, r in enumerate(rows):
        index[v, :len(r)] = r
    return index, np.asarray(cell, np.int64).reshape(-1, 3), np.asarray([len(r) for r in rows], np.int64)


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


# ------------------------------------------------------------------- the cases of tests/test_gpu_pillars_edges.py
# Every input is seeded from cloud / synth; tests/test_pillars_cpu.py walks the same tables and pins voxelize_index (what
# the GPU is compared with) to voxelize_loop on each of them.
#
# The key-width table: name -> (voxel_size, pc_range, grid, B, B * cells, radix passes). `none` = B * cells sorts behind
# every real key and sets the number of 8-bit passes: 1 (the result ends in the second ping-pong buffer), 2, 3 (the
# production pillar grid) and 4, with `none` on and one short of a power of 256, and keys up to bit 30.
KEY_N, KEY_B_N, KEY_C, KEY_MAX_POINTS, KEY_MAX_VOXELS = 9001, 3000, 5, 7, 3000
KEY_WIDTHS = {
    "one_pass": ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 4.0, 4.0, 1.0), (4, 4, 1), 3, 48, 1),
    "2^8-1": ((0.5, 0.25, 1.0), (-1.0, 0.0, -2.0, 1.5, 4.25, 1.0), (5, 17, 3), 1, 255, 1),
    "2^8": ((0.5, 0.5, 4.0), (0.0, -4.0, -3.0, 8.0, 4.0, 1.0), (16, 16, 1), 1, 256, 2),
    "2^16-1": ((0.25, 0.25, 4.0), (0.0, 0.0, -3.0, 63.75, 64.25, 1.0), (255, 257, 1), 1, 65535, 2),
    "2^16": ((0.25, 0.25, 4.0), (-32.0, -32.0, -3.0, 32.0, 32.0, 1.0), (256, 256, 1), 1, 65536, 3),
    "production": ((0.32, 0.32, 6.0), (-74.88, -74.88, -2.0, 74.88, 74.88, 4.0), (468, 468, 1), 4, 876096, 3),
    "2^24": ((0.25,) * 3, (-32.0,) * 3 + (32.0,) * 3, (256, 256, 256), 1, 1 << 24, 4),
    "top": ((0.125,) * 3, (-64.0, -64.0, -32.0, 64.0, 64.0, 32.0), (1024, 1024, 512), 3, 3 << 29, 4),
}
PRODUCTION = dict(voxel_size=(0.32, 0.32, 6.0), pc_range=(-74.88, -74.88, -2.0, 74.88, 74.88, 4.0), max_points=20, C=5)


def sort_passes(B, grid):
    """-> (none = B * cells, the 8-bit passes of the voxeliser's sort) as launch_voxelize forms them: as many bits as
    `none` itself needs, since it has to sort behind every real key"""
    none = int(B) * int(np.prod(np.asarray(grid, np.int64)))
    bits = 0
    while bits < 32 and (1 << bits) <= none:
        bits += 1
    return none, (bits + 7) // 8


def key_width_case(name):
    """-> (points, offsets (B + 1), cfg): one cloud of KEY_N points, or B clouds of KEY_B_N with different tags"""
    vs, rng, _, B, _, _ = KEY_WIDTHS[name]
    cfg = dict(voxel_size=vs, pc_range=rng, max_points=KEY_MAX_POINTS, C=KEY_C)
    if B == 1:
        return cloud("key/" + name, KEY_N, cfg, KEY_C), np.array([0, KEY_N], np.int64), cfg
    parts = [cloud(f"key/{name}/{b}", KEY_B_N, cfg, KEY_C) for b in range(B)]
    return np.concatenate(parts), np.arange(B + 1, dtype=np.int64) * KEY_B_N, cfg


RUN_N, RUN_SMALL_AT = 9001, (0, 4096, 9000)
RUN_BIG_CELL, RUN_SMALL_CELL = (5, 7), (20, 3)              # (x, y) on PILLAR's grid
RUN_MAX_POINTS = (1, 64, 5000, 10000)


def run_length_points():
    """RUN_N points of PILLAR's grid, all in range: those at RUN_SMALL_AT sit mid-cell in one cell, every other one
    mid-cell in another, whose run spans three sort chunks of 4096. Column 3 is the point's index. The small cell has
    the smaller key, so its run starts at sorted entry 0 and the large one ends at entry N."""
    lo, vs = np.asarray(PILLAR["pc_range"][:3], np.float64), np.asarray(PILLAR["voxel_size"], np.float64)
    pts = np.zeros((RUN_N, 5), np.float32)
    pts[:, :2] = lo[:2] + (np.asarray(RUN_BIG_CELL) + 0.5) * vs[:2]
    pts[list(RUN_SMALL_AT), :2] = lo[:2] + (np.asarray(RUN_SMALL_CELL) + 0.5) * vs[:2]
    pts[:, 2] = lo[2] + 0.5 * vs[2]
    pts[:, 3] = np.arange(RUN_N)
    pts[:, 4] = 0.5
    return pts


BIG_B, BIG_N, BIG_HEAD, BIG_TAIL, BIG_CAP = 300, 6000, 5, 11, 40
BIG_SIZES = (0, 0, 1, 37, 0, 255, 256, 257, 3)
BIG_ACTIVE = ((0, 45), (256, 300))      # the samples that take sizes from the cycle; those between are a run of empty ones


def many_samples():
    """-> (points (BIG_N, 5), offsets (BIG_B + 1)): sample sizes cycle through BIG_SIZES over the samples of BIG_ACTIVE
    (so that samples behind the 256th, which the offsets kernel's second stride serves, hold points and hit the cap),
    cut off where the points run out; BIG_HEAD points in front of offsets[0] and BIG_TAIL behind offsets[B] belong to no
    sample and are in range, so that they show if they are not dropped."""
    sizes = np.zeros(BIG_B, np.int64)
    for a, b in BIG_ACTIVE:
        sizes[a:b] = [BIG_SIZES[(i - a) % len(BIG_SIZES)] for i in range(a, b)]
    room = BIG_N - BIG_HEAD - BIG_TAIL
    ends = np.minimum(np.cumsum(sizes), room)
    off = BIG_HEAD + np.concatenate([[0], ends]).astype(np.int64)
    pts = cloud("many_samples", BIG_N, PILLAR, 5)
    lo, vs = np.asarray(PILLAR["pc_range"][:3], np.float64), np.asarray(PILLAR["voxel_size"], np.float64)
    stray = np.r_[0:BIG_HEAD, BIG_N - BIG_TAIL:BIG_N]
    pts[stray, :3] = (lo + (np.stack([stray % 29, stray % 31, 0 * stray], 1) + 0.5) * vs).astype(np.float32)
    return pts, off


OVERFLOW_N, OVERFLOW_CAP = 6000, 50
OVERFLOW_OFFSETS = ((0, 3000, 6000), (0, 4, 9))     # the device's offsets: more, and fewer, points than the host's (0, 10, 20)


def in_range_points(tag, n):
    """n seeded points of PILLAR's range, every one in it"""
    lo, hi = np.asarray(PILLAR["pc_range"][:3]), np.asarray(PILLAR["pc_range"][3:])
    u = synth.uniform(SEED, "pillars/" + tag, (n, 5), 0.0, 1.0)
    u[:, :3] = lo + (0.001 + 0.998 * u[:, :3]) * (hi - lo)
    return u.astype(np.float32)


FAR_P, FAR_AT = 64, (0, 1, 233, 234, 466, 467)


def far_pillars():
    """-> (voxels (FAR_P, 20, 5), num_points, coordinates (P, 4) [b, z, y, x]) on PRODUCTION's 468 x 468 grid with x and y
    indices from FAR_AT: a point's x and y are its pillar's centre +- up to half a cell, so that at index 467 the
    decoration x - (coor * vx + x_offset) cancels 74 m against 74 m"""
    cfg = PRODUCTION
    T, C = cfg["max_points"], cfg["C"]
    lo, hi = np.asarray(cfg["pc_range"][:3], np.float64), np.asarray(cfg["pc_range"][3:], np.float64)
    vs = np.asarray(cfg["voxel_size"], np.float64)
    pairs = [(y, x) for y in FAR_AT for x in FAR_AT]
    p = np.arange(FAR_P)
    yx = np.asarray([pairs[i % len(pairs)] for i in p], np.int64)
    co = np.stack([p // len(pairs), np.zeros(FAR_P, np.int64), yx[:, 0], yx[:, 1]], 1).astype(np.int32)
    u = synth.uniform(SEED, "far", (FAR_P, T, C), 0.0, 1.0)
    vox = u.copy()
    vox[:, :, 0] = lo[0] + (yx[:, 1:2] + 0.5 + (u[:, :, 0] - 0.5) * 0.998) * vs[0]
    vox[:, :, 1] = lo[1] + (yx[:, 0:1] + 0.5 + (u[:, :, 1] - 0.5) * 0.998) * vs[1]
    vox[:, :, 2] = lo[2] + u[:, :, 2] * (hi[2] - lo[2])
    num = (1 + (p * 7) % T).astype(np.int32)
    num[:3] = [1, T, T - 1]
    vox = vox.astype(np.float32)
    vox[np.arange(T)[None, :] >= num[:, None]] = 0
    return vox, num, co


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
# test_gpu_pillars.py and tests/test_gpu_pillars_edges.py in one session) x at most 2, rounded up to one significant
# digit, and under a tenth of the smallest planted-fault ratio of tests/test_pillars_cpu.py (3.4e3); a bar comes down
# or stays, it does not go up. They were first set without an MI355X run, at 4 each, on reasoning: kernel and yardstick
# are fp32 evaluations of the same chain of <= 64-term dot products; the kernel rounds every folded weight once more
# (the rms error of a term grows by at most sqrt(2)) and sums in another order (the same bound), and the per-channel
# measures are maxima over 64 channels of a few hundred rows, which move by about 2x between two equally good
# evaluations: 4 = sqrt(2) x 2, rounded up. The first run on an MI355X (17 rows, the far corner of the production grid
# among them) recorded at worst tensor 1.34 (reader1), chan_rms 2.17 (rows64/c6/l1) and chan_max 1.96 (rows1/c3/l2):
# x 2 gives 2.7 -> 3, 4.3 (the bar stays at 4 = 1.8 x the worst) and 3.9 -> 4.
BARS = {"tensor": 3.0, "chan_rms": 4.0, "chan_max": 4.0}
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
