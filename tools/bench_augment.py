#!/usr/bin/env python3
"""Measure the training input (3dal_pytorch_amd/augment.py: dal3_gt_paste_select, dal3_augment_points, dal3_augment_boxes) and
write profiles/bench_augment.json:

    python tools/bench_augment.py [--batches 1 4] [--iters 30] [--warmup 5] [--out profiles/bench_augment.json]

B in --batches samples of 180 k scene points with 5 features and 20 annotated boxes, 35 candidates a sample from a synthetic
object database of about 200 points an object (resident on the device): `Preprocess` alone and `train_example` (Preprocess ->
voxelize on the 0.1 m grid -> AssignLabel), beside the YARDSTICK: the same formulation in stock PyTorch-ROCm ops on the same
GPU and inputs, written below — the pair matrix as batched tensor expressions, a read-back and the serial acceptance on the
host (it has no stock counterpart on the device), index_select for the objects' rows, a matmul for the rotation, argsort of
the (sample, key) pairs and index_select for the shuffle. The reference itself does this stage in numba on DataLoader
workers; numba is not installed on these machines, so no CPU baseline can be produced and none is quoted.

Wall clock around synchronised calls; every shape warmed; the two alternate inside one process; medians and spreads are
recorded. `dal3_augment_points` (with its sort) is also timed alone between device events and set against the bytes it must
move, rows x F x 4 read plus written, over the 8 TB/s HBM figure. No ratio is fixed in advance."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

augment = importlib.import_module("3dal_pytorch_amd.augment")
center_loss = importlib.import_module("3dal_pytorch_amd.center_loss")
hip = importlib.import_module("3dal_pytorch_amd._hip")

CLASS_NAMES = ["VEHICLE", "PEDESTRIAN", "CYCLIST"]
SIZES = {"VEHICLE": (2.0, 4.5, 1.6), "PEDESTRIAN": (0.8, 0.9, 1.7), "CYCLIST": (0.8, 1.8, 1.6)}
GT_PER_CLASS = {"VEHICLE": 10, "PEDESTRIAN": 6, "CYCLIST": 4}
GROUPS = [{"VEHICLE": 25}, {"PEDESTRIAN": 16}, {"CYCLIST": 14}]          # 15 + 10 + 10 = 35 candidates beside those annotations
PC_RANGE, VOXEL = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0], [0.1, 0.1, 0.15]
N_SCENE, F, DB_OBJECTS, MAX_OBJS, HBM_TBS = 180000, 5, 80, 500, 8.0


def boxes_of(rs, names):
    out = np.zeros((len(names), 9), np.float32)
    for i, n in enumerate(names):
        w, l, h = SIZES[n]
        out[i] = [rs.uniform(-70, 70), rs.uniform(-70, 70), rs.uniform(-1, 1), w, l, h, rs.uniform(-3, 3), rs.uniform(-3, 3), rs.uniform(-3.1, 3.1)]
    return out


def write_database(root):
    import pickle
    rs = np.random.RandomState(5)
    os.makedirs(os.path.join(root, "db"))
    infos = {}
    for name in CLASS_NAMES:
        b = boxes_of(rs, [name] * DB_OBJECTS)
        infos[name] = []
        for i in range(DB_OBJECTS):
            n = int(rs.randint(150, 251))
            path = f"db/{name}_{i}.bin"
            (rs.standard_normal((n, F)) * 0.5).astype(np.float32).tofile(os.path.join(root, path))
            infos[name].append(dict(name=name, path=path, box3d_lidar=b[i], num_points_in_gt=n, difficulty=0))
    with open(os.path.join(root, "dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f)
    return os.path.join(root, "dbinfos.pkl")


def corners(b):
    """(n, 9) -> (n, 4, 2), center_to_corner_box2d in stock ops"""
    norm = torch.tensor([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]], device=b.device)
    c = b[:, None, 3:5] * norm[None]
    sn, cs = torch.sin(b[:, 8])[:, None], torch.cos(b[:, 8])[:, None]
    return torch.stack([c[..., 0] * cs + c[..., 1] * sn, -c[..., 0] * sn + c[..., 1] * cs], -1) + b[:, None, :2]


def stock_pairs(cand, total):
    """box_collision_test's matrix (nc, n) as tensor expressions"""
    a, q = corners(cand), corners(total)
    lo_a, hi_a, lo_q, hi_q = a.min(1).values, a.max(1).values, q.min(1).values, q.max(1).values
    stand = ((torch.minimum(hi_a[:, None], hi_q[None]) - torch.maximum(lo_a[:, None], lo_q[None])) > 0).all(-1)
    A, Bp = a[:, None, :, None], a.roll(-1, 1)[:, None, :, None]         # (nc, 1, 4, 1, 2)
    C, D = q[None, :, None, :], q.roll(-1, 1)[None, :, None, :]          # (1, n, 1, 4, 2)

    def ccw(P, Q, R):
        return (R[..., 1] - P[..., 1]) * (Q[..., 0] - P[..., 0]) > (Q[..., 1] - P[..., 1]) * (R[..., 0] - P[..., 0])
    cross = ((ccw(A, C, D) != ccw(Bp, C, D)) & (ccw(A, Bp, C) != ccw(A, Bp, D))).flatten(2).any(-1)

    def inside(out, inn):                                               # every corner of inn strictly inside out
        vec = -(out - out.roll(-1, 1))                                  # (no, 4, 2)
        d = out[:, None, :, None] - inn[None, :, None, :]               # (no, ni, 4 edges, 4 corners, 2)
        c = vec[:, None, :, None, 1] * d[..., 0] - vec[:, None, :, None, 0] * d[..., 1]
        return (c < 0).flatten(2).all(-1)
    return stand & (cross | inside(a, q) | inside(q, a).T)


def stock_step(st):
    """the yardstick: one batch in stock PyTorch-ROCm ops (the same inputs, draws and candidates)"""
    B, dev = st["B"], st["dev"]
    ok_all, segs, gts = [], [], []
    for b in range(B):
        ng = int(st["gt_cnt"][b])
        total = torch.cat([st["gt_boxes"][b, :ng], st["cand_boxes"][b]])
        m = stock_pairs(st["cand_boxes"][b], total).cpu().numpy()       # the read-back the serial acceptance needs
        nc, group = m.shape[0], st["group"][b]
        m[np.arange(nc), ng + np.arange(nc)] = False
        ok, rej = np.zeros(nc, bool), np.zeros(nc, bool)
        for i in range(nc):
            live = np.ones(ng + nc, bool)
            live[ng:] = np.where(group < group[i], ok, np.where(group == group[i], ~rej, False))
            rej[i] = bool((m[i] & live).any())
            ok[i] = not rej[i]
        ok_all.append(ok)
        okd = torch.from_numpy(ok).to(dev)
        rows = st["db"].points.index_select(0, st["row_index"][b])
        rows = torch.cat([rows[:, :3] + st["cand_boxes"][b].index_select(0, st["row_cand"][b])[:, :3], rows[:, 3:]], 1)
        rows = torch.where(okd.index_select(0, st["row_cand"][b])[:, None], rows, torch.full_like(rows, float("nan")))
        p = torch.cat([rows, st["scene"][b]])
        x = st["xform"][b]
        flip = torch.ones(3, device=dev)
        flip[1], flip[0] = 1 - 2 * x[0].float(), 1 - 2 * x[1].float()
        sn, cs = torch.sin(x[2]).float(), torch.cos(x[2]).float()
        rot = torch.stack([torch.stack([cs, -sn, sn * 0]), torch.stack([sn, cs, sn * 0]), torch.tensor([0.0, 0.0, 1.0], device=dev)])
        xyz = ((p[:, :3] * flip) @ rot) * x[3].float() + x[4:].float()
        segs.append(torch.cat([xyz, p[:, 3:]], 1))
        g = torch.cat([st["gt_boxes"][b, :ng], st["cand_boxes"][b][okd]])
        gx = ((g[:, :3] * flip) @ rot) * x[3].float() + x[4:].float()
        gts.append(torch.cat([gx, g[:, 3:6] * x[3].float(), g[:, 6:]], 1))
    pts = torch.cat(segs)
    order = torch.argsort(st["sample_of_row"] * (2 ** 31) + st["keys"].long(), stable=True)
    return pts.index_select(0, order), ok_all, gts


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    v = np.asarray(v)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "p90_ms": float(np.percentile(v, 90)), "n": int(v.size)}


def bench(B, a, db, dev):
    rs = np.random.RandomState(10 + B)
    names = [n for n, k in GT_PER_CLASS.items() for _ in range(k)]
    max_gt = len(names)
    gt_boxes = np.stack([boxes_of(rs, names) for _ in range(B)])
    gt_cls = np.tile(np.array([CLASS_NAMES.index(n) + 1 for n in names], np.int32), (B, 1))
    gt_cnt = np.full(B, max_gt, np.int32)
    scene = np.concatenate([rs.uniform(-75, 75, (B * N_SCENE, 2)), rs.uniform(-2, 4, (B * N_SCENE, 1)), rs.uniform(0, 1, (B * N_SCENE, F - 3))], 1)
    pts = torch.from_numpy(scene.astype(np.float32)).to(dev)
    off = np.arange(B + 1) * N_SCENE
    sampler = augment.DataBaseSamplerV2(db, GROUPS, rng=np.random.RandomState(1))
    cfg = dict(mode="train", shuffle_points=True, global_rot_noise=0.78539816, global_scale_noise=[0.95, 1.05], global_translate_std=0.5,
               class_names=CLASS_NAMES, db_sampler=sampler)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    pre = augment.Preprocess(cfg, pc_range=PC_RANGE, max_objs=MAX_OBJS, generator=gen)
    cands = pre.candidates(gt_cls, gt_cnt)
    assert all(len(c) == 35 for c in cands)
    gtd = torch.from_numpy(gt_boxes).to(dev)
    n = B * N_SCENE + sum(int(db.offsets[i + 1] - db.offsets[i]) for c in cands for i, _, _ in c)
    draws = augment.make_draws(B, n, 0.78539816, [0.95, 1.05], 0.5, gen, dev)
    acfg = dict(out_size_factor=8, gaussian_overlap=0.1, max_objs=MAX_OBJS, min_radius=2,
                target_assigner=dict(tasks=[dict(num_class=3, class_names=CLASS_NAMES)]))
    assigner = center_loss.AssignLabel(cfg=acfg)

    def mine():
        return pre(pts, off, gtd, gt_cls, gt_cnt, draws, cands)

    def chain():
        return augment.train_example(pre, assigner, pts, off, gtd, gt_cls, gt_cnt, voxel_size=VOXEL, pc_range=PC_RANGE, max_points=5,
                                     max_voxels=150000, draws=draws, candidates=cands)
    # the yardstick's inputs, prepared once as Preprocess prepares its own on the host
    st = dict(B=B, dev=dev, db=db, gt_boxes=gtd, gt_cnt=gt_cnt, xform=draws.xform, keys=draws.keys, cand_boxes=[], group=[], row_index=[],
              row_cand=[], scene=[pts[off[b]:off[b + 1]] for b in range(B)])
    sample_of_row = []
    for b, c in enumerate(cands):
        idx = np.array([i for i, _, _ in c])
        st["cand_boxes"].append(db.boxes.index_select(0, torch.from_numpy(idx).to(dev)))
        st["group"].append(np.array([g for _, _, g in c]))
        st["row_index"].append(torch.from_numpy(np.concatenate([np.arange(db.offsets[i], db.offsets[i + 1]) for i in idx])).to(dev))
        st["row_cand"].append(torch.from_numpy(np.concatenate([np.full(db.offsets[i + 1] - db.offsets[i], k) for k, i in enumerate(idx)])).to(dev))
        sample_of_row.append(np.full(len(st["row_index"][-1]) + N_SCENE, b))
    st["sample_of_row"] = torch.from_numpy(np.concatenate(sample_of_row)).to(dev)
    # the points entry alone, between device events
    lib, events = hip.lib(), []
    inner = lib.dal3_augment_points

    def timed(args, stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = inner(args, stream)
        e1.record()
        events.append((e0, e1))
        return rc
    for _ in range(a.warmup):
        out, ok_stock, _ = stock_step(st)
        got = mine()
        chain()
    torch.cuda.synchronize()
    ok_mine = pre.last["accept"].cpu().numpy().astype(bool)
    agree = all(np.array_equal(ok_mine[b, :35], ok_stock[b]) for b in range(B))
    valid = ~torch.isnan(got[0][:, 0])
    err = float((got[0][valid] - out[valid]).abs().max()) if agree else None
    w = {k: [] for k in ("preprocess", "train_example", "stock")}
    lib.dal3_augment_points = timed
    try:
        for _ in range(a.iters):
            w["preprocess"].append(wall(mine)[0])
            w["stock"].append(wall(lambda: stock_step(st))[0])
            w["train_example"].append(wall(chain)[0])
    finally:
        lib.dal3_augment_points = inner
    torch.cuda.synchronize()
    ev = [e0.elapsed_time(e1) for e0, e1 in events]
    moved = 2 * n * F * 4
    return {"B": B, "source_rows": n, "candidates_per_sample": 35, "accepted": [int(v.sum()) for v in ok_stock], "accept_flags_agree": agree,
            "max_abs_difference_to_stock_points": err, "preprocess": stats(w["preprocess"]), "train_example": stats(w["train_example"]),
            "stock_pytorch_preprocess": stats(w["stock"]), "preprocess_over_stock": float(np.median(w["preprocess"]) / np.median(w["stock"])),
            "augment_points_device": dict(stats(ev), bytes_read_plus_written=moved, floor_ms_at_hbm_rate=moved / (HBM_TBS * 1e12) * 1e3,
                                          launches=3 * (4 + (1 if B > 1 else 0)) + 2)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_augment.json"))
    a = p.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "augment", "device": torch.cuda.get_device_name(0), "scene_points": N_SCENE, "features": F, "iters": a.iters, "warmup": a.warmup,
           "timing": "wall clock around synchronised calls, Preprocess and the stock formulation alternating inside one process; the points entry between device events",
           "baseline": "the same formulation in stock PyTorch-ROCm ops on the same GPU (tensor pair matrix, read-back, host acceptance, index_select, matmul, argsort)",
           "cpu_numba_baseline": "none: numba is not installed on these machines, the reference's DataLoader-worker timing cannot be produced",
           "step": []}
    with tempfile.TemporaryDirectory() as root:
        db = augment.GTDatabase(write_database(root), root, F, (), dev)
        for B in a.batches:
            res["step"].append(bench(B, a, db, dev))
            print(json.dumps(res["step"][-1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
