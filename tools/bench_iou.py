#!/usr/bin/env python3
"""tools/bench_iou.py — the rotated-box IoU kernels (3dal_pytorch_amd/iou.py -> dal3_box_iou_*) on one GPU, and what
the 16-bit arithmetic paths do to box quality, written to a JSON file (never printed on bench.py's line).

  python tools/bench_iou.py [--out profiles/bench_iou.json] [--reps 20] [--warmup 3]

  pairwise   512 x 512, 4096 x 4096, 16384 x 4096 boxes, float32; "scene": boxes scattered like a busy lidar scene
             (most pairs disjoint, exact 0 from the bounding-circle test), "overlap": every box within a metre of the
             origin (every pair clipped). Median of HIP-event-timed launches -> pairs/s. For the scene inputs also the
             divergence the early exit leaves, counted on the host from the same boxes and the kernel's lane map (a wave
             = one row of a x 64 consecutive columns of b): the share of waves with at least one clipped pair, and the
             share of lanes in those waves that clip.
  paired     1 M near-overlapping pairs (the eval metric's kernel), float32 and float64.
  precision  the bench workload (C2: 4096 static crops x 1024 points) on the fp32 path and on the f16x3 / fp16 / bf16
             arithmetic paths (free-running: own mask, own draws); each path's boxes against the fp32 path's boxes:
             mean 3D IoU, its median, the share below 0.7, and the same for the BEV IoU. The bench's synthetic weights
             decode most crops to a non-positive size (an empty box to the IoU), so the figures are also given with
             every size taken in absolute value.
"""
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
from bench_workloads import make_static                     # noqa: E402

arch = importlib.import_module("3dal_pytorch_amd.arch")
iou = importlib.import_module("3dal_pytorch_amd.iou")
WAVE = 64                                                   # columns of b per wave (dal3_iou.hip IOU_TB)


def scene_boxes(n, seed, extent=150.0):
    rng = np.random.default_rng(seed)
    size = np.array(arch.MEAN_SIZE)[rng.integers(0, 3, n)] * rng.uniform(0.8, 1.2, (n, 3))
    return np.concatenate([rng.uniform(-extent / 2, extent / 2, (n, 2)), rng.normal(0, 0.5, (n, 1)), size,
                           rng.uniform(-np.pi, np.pi, (n, 1))], 1)


def overlap_boxes(n, seed):
    b = scene_boxes(n, seed)
    b[:, :2] = np.random.default_rng(seed + 1).uniform(-1, 1, (n, 2))
    return b


def time_call(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    return ms[len(ms) // 2], ms[0]


def divergence(a, b):
    """waves (row i, 64-column block of b) with >= 1 pair past the bounding-circle test, and the lanes that clip in them"""
    ra = np.hypot(a[:, 3], a[:, 4]) / 2
    rb = np.hypot(b[:, 3], b[:, 4]) / 2
    m = b.shape[0]
    pad = -m % WAVE
    waves_busy = lanes_busy = waves = 0
    for s in range(0, a.shape[0], 512):
        blk = a[s:s + 512]
        d2 = (blk[:, None, 0] - b[None, :, 0]) ** 2 + (blk[:, None, 1] - b[None, :, 1]) ** 2
        near = d2 <= ((ra[s:s + 512, None] + rb[None, :]) * 1.000001) ** 2
        near = np.pad(near, ((0, 0), (0, pad))).reshape(blk.shape[0], -1, WAVE)
        per_wave = near.sum(2)
        waves += per_wave.size
        waves_busy += int((per_wave > 0).sum())
        lanes_busy += int(per_wave.sum())
    return {"waves": waves, "waves_with_a_clipped_pair": waves_busy,
            "share_of_waves_that_clip": round(waves_busy / waves, 5),
            "lanes_clipping_in_those_waves": round(lanes_busy / max(waves_busy * WAVE, 1), 4),
            "pairs_clipped": lanes_busy, "share_of_pairs_clipped": round(lanes_busy / (a.shape[0] * m), 6)}


def pairwise_leg(dev, reps, warmup):
    out = []
    for n, m in ((512, 512), (4096, 4096), (16384, 4096)):
        for kind in ("scene", "overlap"):
            gen = scene_boxes if kind == "scene" else overlap_boxes
            a_np, b_np = gen(n, 10), gen(m, 20)
            a = torch.from_numpy(a_np).float().to(dev)
            b = torch.from_numpy(b_np).float().to(dev)
            med, best = time_call(lambda: iou.boxes_iou_bev_3d(a, b), reps, warmup)
            r = {"n": n, "m": m, "boxes": kind, "dtype": "float32", "outputs": "bev+3d", "ms_median": round(med, 4),
                 "ms_min": round(best, 4), "pairs_per_s": round(n * m / (med * 1e-3), 0)}
            medb, _ = time_call(lambda: iou.boxes_iou_bev(a, b), reps, warmup)
            r["ms_median_bev_only"] = round(medb, 4)
            r["out_bytes_per_s_bev_3d"] = round(8 * n * m / (med * 1e-3), 0)
            if kind == "scene":
                r["divergence"] = divergence(a.double().cpu().numpy(), b.double().cpu().numpy())
            out.append(r)
            print(json.dumps(r), flush=True)
    return out


def paired_leg(dev, reps, warmup):
    out = []
    n = 1 << 20
    rng = np.random.default_rng(30)
    a_np = scene_boxes(n, 31, 100.0)
    b_np = np.concatenate([a_np[:, :2] + rng.normal(0, 1, (n, 2)) * a_np[:, 3:5] * 0.5, a_np[:, 2:3],
                           a_np[:, 3:6] * rng.uniform(0.7, 1.3, (n, 3)), a_np[:, 6:7] + rng.normal(0, 0.5, (n, 1))], 1)
    for dt in (torch.float32, torch.float64):
        a, b = torch.from_numpy(a_np).to(dev, dt), torch.from_numpy(b_np).to(dev, dt)
        med, best = time_call(lambda: iou.paired_iou(a, b), reps, warmup)
        r = {"n": n, "dtype": str(dt).replace("torch.", ""), "ms_median": round(med, 4), "ms_min": round(best, 4),
             "pairs_per_s": round(n / (med * 1e-3), 0),
             "share_of_pairs_overlapping": round(float((iou.paired_iou(a, b)[0] > 0).float().mean()), 4)}
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def precision_leg(dev):
    model, inputs, _ = make_static(4096, 1024, dev, 0, "fp32")
    with torch.no_grad():
        model.precision = "fp32"
        ref = model._run(*inputs)["boxes7"].double()
        out = {"workload": "StaticModelOneBoxEst, 4096 crops x 1024 points (bench.py C2), fp32-stored points; each path "
                           "free-running (its own mask and draws)", "crops": int(ref.shape[0])}
        # the bench's synthetic (random-init) weights decode most crops to a non-positive size, which the IoU counts as
        # an empty box: the figures are given on the boxes as decoded AND with every size taken in absolute value
        positive = (ref[:, 3:6] > 0).all(1)
        out["crops_with_all_fp32_sizes_positive"] = int(positive.sum())

        def stats(got, want):
            vb, v3 = iou.paired_iou(got, want)
            v3n, vbn = v3.cpu().numpy().astype(np.float64), vb.cpu().numpy().astype(np.float64)
            return {"iou_3d_mean": round(float(np.mean(v3n)), 5), "iou_3d_median": round(float(np.median(v3n)), 5),
                    "iou_3d_below_0.7": round(float(np.mean(v3n < 0.7)), 5),
                    "iou_3d_below_0.9": round(float(np.mean(v3n < 0.9)), 5),
                    "iou_bev_mean": round(float(np.mean(vbn)), 5), "iou_bev_below_0.7": round(float(np.mean(vbn < 0.7)), 5)}

        def absolute(b):
            b = b.clone()
            b[:, 3:6] = b[:, 3:6].abs()
            return b
        for prec in ("f16x3", "fp16", "bf16"):
            model.precision = prec
            got = model._run(*inputs)["boxes7"].double()
            out[prec] = {"as_decoded": stats(got, ref), "sizes_in_absolute_value": stats(absolute(got), absolute(ref)),
                         "centre_shift_m_median": round(float((got[:, :3] - ref[:, :3]).norm(dim=1).median()), 5),
                         "size_rel_change_median": round(float(((got[:, 3:6] - ref[:, 3:6]).abs() /
                                                                 ref[:, 3:6].abs().clamp_min(1e-6)).max(1).values.median()), 5)}
            print(prec, json.dumps(out[prec]), flush=True)
        model.precision = "fp32"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_iou.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_iou.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rec = {"written_by": "tools/bench_iou.py", "taken": time.strftime("%Y-%m-%d %H:%M:%S"),
           "device": torch.cuda.get_device_name(0), "timing": f"HIP events around each launch, {a.warmup} warm-up, "
                                                             f"median of {a.reps}"}
    rec["pairwise"] = pairwise_leg(dev, a.reps, a.warmup)
    rec["paired"] = paired_leg(dev, a.reps, a.warmup)
    rec["precision_vs_fp32_boxes"] = precision_leg(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
