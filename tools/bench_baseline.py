#!/usr/bin/env python3
"""The baseline runs' scoring at the size of a Waymo validation split (of the order of 10^6 (track, frame) samples:
~200 segments x ~200 frames x tens of tracks), on synthetic tables. Times, on the current GPU:
  score_tracks   (a) baseline.score_tracks alone — dal3_score_tracks with its accumulator, tables already on the
                 device: HIP events around the call, median of --reps after a warm-up;
  host_route     (b) the same samples through what the package offered for this job before: the two boxes per sample
                 built on the host with eval.py's vectorised NumPy (transform_box, the size / heading class round
                 trips: the arithmetic of eval.metric_samples), uploaded, iou.paired_iou on the device (HIP events:
                 upload and kernel), then the NumPy threshold and sums of eval.box_metrics on the downloaded values;
                 each part timed, and its result checked against (a)'s accumulator;
  flatten        baseline.flatten (the host work that remains in front of (a)) on --flatten_samples samples of
                 in-memory tracks and annotations (no pickle reads), scaled to the split.
One JSON line; --out writes it to a file.
    python tools/bench_baseline.py [--samples 1000000 --reps 20 --out profiles/bench_baseline.json]
"""
import argparse
import datetime
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
baseline = importlib.import_module("3dal_pytorch_amd.baseline")
ev = importlib.import_module("3dal_pytorch_amd.eval")
iou = importlib.import_module("3dal_pytorch_amd.iou")
arch = importlib.import_module("3dal_pytorch_amd.arch")


def tables(S, seed, n_frames=40000):
    """flat dal3_score_tracks tables: vehicle-frame boxes carried to the global frame by their frame's pose, a ground
    truth a fraction of the box's size away (float32, the annotations' dtype), 10 % of the samples without GT"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-np.pi, np.pi, n_frames)
    pose = np.tile(np.eye(4), (n_frames, 1, 1))
    pose[:, 0, 0], pose[:, 0, 1], pose[:, 1, 0], pose[:, 1, 1] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)
    pose[:, :3, 3] = rng.uniform(-5e3, 5e3, (n_frames, 3)) * [1, 1, 0.01]
    frame = rng.integers(0, n_frames, S).astype(np.int32)
    size = np.array(arch.MEAN_SIZE)[rng.integers(0, 3, S)] * rng.uniform(0.7, 1.3, (S, 3))
    local = np.concatenate([rng.uniform(-50, 50, (S, 2)), rng.uniform(-1, 1, (S, 1))], 1)
    yaw = rng.uniform(-np.pi, np.pi, S)
    centre = np.einsum("sij,sj->si", pose[frame][:, :3, :3], local) + pose[frame][:, :3, 3]
    gt = np.concatenate([local + rng.normal(0, 1, (S, 3)) * np.concatenate([size[:, :2] * 0.3, np.full((S, 1), 0.2)], 1),
                         size * rng.uniform(0.8, 1.25, (S, 3)), (yaw + rng.normal(0, 0.3, S))[:, None]], 1)
    return {"boxes": np.concatenate([centre, size, (yaw + ang[frame])[:, None]], 1), "box_row": np.arange(S, dtype=np.int32),
            "frame": frame, "pose_inv": np.linalg.inv(pose).reshape(-1, 16), "gt": gt.astype(np.float32),
            "has_gt": (rng.uniform(0, 1, S) > 0.1).astype(np.uint8),
            "type": rng.choice(np.array([1, 2, 4], np.int32), S, p=[0.65, 0.2, 0.15])}


def events(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def host_boxes(t):
    """the scored samples' (pred, label) float64 boxes by eval.py's NumPy: what eval.metric_samples does per run"""
    k = t["has_gt"] != 0
    init = ev._transform(t["boxes"][t["box_row"][k]], t["pose_inv"][t["frame"][k]].reshape(-1, 4, 4))
    gt = t["gt"][k]
    pred = np.concatenate([init[:, :3], ev._size_class_round_trip(init[:, 3:6]), np.zeros((len(init), 1))], 1)
    label = np.concatenate([gt[:, :3].astype(np.float64), ev._size_class_round_trip(gt[:, 3:6].astype(np.float64)),
                            ev._angle_class_round_trip(gt[:, 6] - init[:, 6])[:, None]], 1)
    return pred, label, k


class MemoryAnnos:
    """eval.Annos over annotation dicts held in memory"""

    def __init__(self, annos):
        self.annos = annos

    def __call__(self, token):
        return self.annos[token]


def flatten_input(S, seed, frames_per_track=200, objects=25):
    rng = np.random.default_rng(seed)
    n_tracks = max(1, S // frames_per_track)
    n_seg = max(1, n_tracks // objects)
    annos, track = {}, {}
    for s in range(n_seg):
        for f in range(frames_per_track):
            annos[f"s{s}_f{f}"] = {"veh_to_global": np.eye(4).reshape(16) + 0.0,
                                   "objects": [{"name": f"o{k}", "box": rng.normal(0, 1, 9).astype(np.float32)}
                                               for k in range(objects) if (k + f) % 10]}
    for i in range(n_tracks):
        s, k = (i // objects) % n_seg, i % objects
        track[f"{i:032x}"] = {"type": [1] * frames_per_track, "bbox": list(rng.normal(0, 1, (frames_per_track, 7))),
                              "score": list(rng.uniform(0, 1, frames_per_track).astype(np.float32)),
                              "match": [f"o{k}"] * frames_per_track, "token": [f"s{s}_f{f}" for f in range(frames_per_track)]}
    return track, MemoryAnnos(annos)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--flatten_samples", type=int, default=200_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    S = a.samples
    t = tables(S, 31)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in t.items()}

    # (a) the kernel alone
    acc = baseline.ScoreAccumulator(dev)
    run = lambda: baseline.score_tracks(d["boxes"], d["box_row"], d["frame"], d["pose_inv"], d["gt"], d["has_gt"],   # noqa: E731
                                        d["type"], acc=acc)
    for _ in range(3):
        run()
    acc.reset()
    vb, v3 = run()
    torch.cuda.synchronize()
    mine = acc.result()
    kernel = events(run, max(a.reps, 20))
    in_bytes = 7 * 8 + 4 + 4 + 7 * 4 + 1 + 4 + 8                      # per sample: box, row, frame, gt, flag, type, outputs

    # (b) the host-built boxes -> paired_iou -> NumPy
    t0 = time.perf_counter()
    pred, label, k = host_boxes(t)
    t_build = (time.perf_counter() - t0) * 1e3
    out = {}

    def device_part():
        out["v"] = iou.paired_iou(torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev))
    device_part()
    dev_ms = events(device_part, max(a.reps, 20))
    pd, ld = torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev)
    pair_ms = events(lambda: iou.paired_iou(pd, ld), max(a.reps, 20))
    t0 = time.perf_counter()
    hb, h3 = out["v"][0].cpu().numpy(), out["v"][1].cpu().numpy()
    thr = np.where(t["type"][k] == 1, 0.7, 0.5)
    n_pass = int(np.sum(h3 >= thr))
    sums = (float(np.sum(hb, dtype=np.float64)), float(np.sum(h3, dtype=np.float64)))
    t_reduce = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(h3.view(np.uint32), v3.cpu().numpy()[k].view(np.uint32)))
    agree = {"iou_bits_equal": same, "pass_equal": n_pass == mine["n_iou_3d_pass"],
             "sum_3d_rel_diff": abs(sums[1] - mine["sum_iou_3d"]) / max(abs(sums[1]), 1e-30)}

    # the flattening in front of (a)
    track, annos = flatten_input(a.flatten_samples, 32)
    t0 = time.perf_counter()
    flat = baseline.flatten(track, annos)
    t_flat = (time.perf_counter() - t0) * 1e3

    rec = {"bench": "baseline", "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "samples": S, "scored": int(k.sum()), "reps": max(a.reps, 20),
           "score_tracks": {"ms": round(kernel[0], 4), "ms_min": round(kernel[1], 4), "ms_max": round(kernel[2], 4),
                            "samples_per_s": round(S / (kernel[0] * 1e-3)), "bytes_per_sample": in_bytes,
                            "GB_per_s": round(S * in_bytes / (kernel[0] * 1e-3) / 1e9, 1)},
           "host_route": {"build_boxes_host_ms": round(t_build, 1),
                          "upload_and_paired_iou_ms": round(dev_ms[0], 4), "paired_iou_ms": round(pair_ms[0], 4),
                          "download_threshold_sum_host_ms": round(t_reduce, 1),
                          "total_ms": round(t_build + dev_ms[0] + t_reduce, 1)},
           "agreement": agree,
           "flatten": {"samples": int(flat["n_samples"]), "ms": round(t_flat, 1),
                       "split_estimate_ms": round(t_flat * S / max(flat["n_samples"], 1), 0)},
           "means": {"iou2d": round(mine["iou2d"], 6), "iou3d": round(mine["iou3d"], 6), "acc": round(mine["acc"], 6)}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
