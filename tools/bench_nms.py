#!/usr/bin/env python3
"""The detector's post-processing at the size of a Waymo sequence: --frames x --tasks segments of ~4096 candidates from
clustered scenes (objects with 1-8 jittered copies, as a centre heatmap's neighbouring cells give). Times, on the
current GPU (CUDA events, median of --reps after a warm-up):
  rotate    dal3_nms, IoU 0.7 / pre 4096 / post 500, all segments in one enqueue
  circle    dal3_nms, circle mode (radius^2 1.0, post 83)
  sort      the same rotate call with post_max = 1: the scan stops after the first block, what is left is the sort and
            the IouBox table; suppress = rotate - sort
  decode    dal3_center_decode at --hw x --hw, --batch samples x --tasks tasks of one class with vel
  baseline  the only route without dal3_nms: per segment torch.sort, the iou.boxes_iou_bev n x n matrix, a download and
            the NumPy greedy scan, on --baseline_segments segments, scaled to all of them (a host time)
and checks the kernel's kept rows against that route on those segments. One JSON line; --out writes it to a file.
    python tools/bench_nms.py [--frames 198 --tasks 3 --reps 5 --out profiles/bench_nms.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
nms = importlib.import_module("3dal_pytorch_amd.nms")
iou = importlib.import_module("3dal_pytorch_amd.iou")
detect = importlib.import_module("3dal_pytorch_amd.detect")
import nms_ref  # noqa: E402


def segment(rng, n):
    """n candidates: objects over 150 m x 150 m, each with 1..8 jittered copies; distinct scores"""
    n_obj = n // 3 + 8
    c = np.concatenate([rng.uniform(-75, 75, (n_obj, 2)), rng.uniform(-1, 1, (n_obj, 1)),
                        rng.uniform([3.5, 1.6, 1.4], [5.5, 2.3, 2.0], (n_obj, 3)), rng.uniform(-np.pi, np.pi, (n_obj, 1))], 1)
    rows = np.repeat(c, rng.integers(1, 9, n_obj), axis=0)[:n]
    assert rows.shape[0] == n
    rows[:, :2] += rng.normal(0, 0.35, (n, 2))
    rows[:, 3:6] *= rng.uniform(0.9, 1.1, (n, 3))
    rows[:, 6] += rng.normal(0, 0.1, n)
    return rows.astype(np.float32), rng.permutation(np.linspace(0.1, 0.99, n)).astype(np.float32)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), [round(t, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=198)
    ap.add_argument("--tasks", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline_segments", type=int, default=6)
    ap.add_argument("--hw", type=int, default=468)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(7)
    F, n = a.frames * a.tasks, a.candidates
    parts = [segment(rng, n) for _ in range(F)]
    boxes = torch.from_numpy(np.concatenate([p[0] for p in parts])).to(dev)
    scores = torch.from_numpy(np.concatenate([p[1] for p in parts])).to(dev)
    off = np.arange(F + 1, dtype=np.int64) * n
    off_dev = torch.from_numpy(off).to(dev)
    cases = {"rotate": lambda: nms.batched_nms(boxes, scores, off, "rotate", 0.7, 4096, 500, seg_offsets_device=off_dev),
             "circle": lambda: nms.batched_nms(boxes, scores, off, "circle", 1.0, 0, 83, seg_offsets_device=off_dev),
             "sort": lambda: nms.batched_nms(boxes, scores, off, "rotate", 0.7, 4096, 1, seg_offsets_device=off_dev)}
    rec = {"bench": "nms", "device": torch.cuda.get_device_name(0), "segments": F, "candidates_per_segment": n, "reps": a.reps}
    for name, fn in cases.items():
        fn()                                                # warm-up
        torch.cuda.synchronize()
        rec[name + "_ms"], rec[name + "_ms_all"] = timed(fn, a.reps)
        rec[name + "_ms"] = round(rec[name + "_ms"], 3)
    rec["suppress_ms"] = round(rec["rotate_ms"] - rec["sort_ms"], 3)
    keep, count = cases["rotate"]()
    count_h = count.cpu().numpy()
    rec["kept_per_segment_mean"] = round(float(count_h.mean()), 1)

    # the route without dal3_nms, on the first segments
    def baseline(f):
        b, s = boxes[off[f]:off[f + 1]], scores[off[f]:off[f + 1]]
        o = torch.sort(s, descending=True, stable=True)[1][:4096]
        m = iou.boxes_iou_bev(b[o], b[o]).cpu().numpy()
        return o.cpu().numpy()[nms_ref.greedy(m > np.float32(0.7), 500)]
    baseline(0)
    q = min(a.baseline_segments, F)
    t0 = time.perf_counter()
    want = [baseline(f) for f in range(q)]
    t_base = (time.perf_counter() - t0) * 1e3
    keep_h = keep[:q].cpu().numpy()
    rec["baseline_ms_per_segment"] = round(t_base / q, 2)
    rec["baseline_ms_all_segments_estimate"] = round(t_base / q * F, 0)
    rec["baseline_equal_on_first_segments"] = bool(all(np.array_equal(keep_h[f, :count_h[f]], want[f]) for f in range(q)))
    rec["ratio_baseline_over_rotate"] = round(t_base / q * F / rec["rotate_ms"], 1)

    # the decode of one batch
    g = np.random.default_rng(11)
    shape = lambda c: (a.batch, c, a.hw, a.hw)              # noqa: E731
    frac = min(1.0, n / float(a.hw * a.hw))                # about n cells per (sample, task) above the threshold
    mu = -2.197 - 1.5 * float(np.sqrt(2) * _erfinv(1 - 2 * frac)) if frac < 1 else 3.0
    tasks = [{k: torch.from_numpy(v.astype(np.float32)).to(dev) for k, v in
              {"hm": g.normal(mu, 1.5, shape(1)), "reg": g.uniform(0, 1, shape(2)), "height": g.normal(0, 2, shape(1)),
               "dim": g.normal(1.0, 0.3, shape(3)), "rot": g.normal(0, 1, shape(2)), "vel": g.normal(0, 3, shape(2))}.items()}
             for _ in range(a.tasks)]
    post = detect.CenterHeadPost(nms_ref.as_test_cfg(nms_ref.CONFIGS["ref"]), [1] * a.tasks)
    r = post.decode(tasks)
    torch.cuda.synchronize()
    t_dec, all_dec = timed(lambda: post.decode(tasks), a.reps)
    post.decode_nms(tasks)
    t_both, all_both = timed(lambda: post.decode_nms(tasks), a.reps)
    rec.update({"decode_hw": a.hw, "decode_batch": a.batch, "decode_tasks": a.tasks,
                "decode_candidates_mean": round(float(r["seg_count"].float().mean().item()), 1),
                "decode_ms": round(t_dec, 3), "decode_ms_all": all_dec, "decode_nms_ms": round(t_both, 3),
                "decode_nms_ms_all": all_both, "decode_status": int(r["status"].item())})
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def _erfinv(y):
    return float(torch.erfinv(torch.tensor(float(y), dtype=torch.float64)).item())


if __name__ == "__main__":
    main()
