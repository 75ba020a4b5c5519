#!/usr/bin/env python3
"""The training run's metric kernel and step (metrics.py, fit.py) on one GPU, one JSON line:

  metric   TrainMetrics.update alone (dal3_box_estimation_metrics: decode + IoU of B pairs + the segmentation count over
           B x N points), HIP-event median per call, at 64 x 4096 (the static step) and 4096 x 1024; run the script
           under `rocprofv3 --kernel-trace --stats` for the kernel's own time;
  step     tools/bench_train.py's step (StaticModelOneBoxEst, 64 x 4096 synthetic crops, Adam) with and without the
           metric update behind it, interleaved, HIP-event medians;
  fit      fit.train_one_epoch on a synthetic segment of 64 x --fit-batches static tracks at batch 64, crops and labels
           from prep on the device: epoch wall time / steps after one warm-up epoch (one sync per epoch).

    python tools/bench_train_metrics.py [--precision fp32|f16x3] [--sampler numpy|device] [--out FILE]
"""
import argparse
import importlib
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
synth = importlib.import_module("3dal_pytorch_amd.synth")
sm = importlib.import_module("3dal_pytorch_amd.static_model")
losses = importlib.import_module("3dal_pytorch_amd.losses")
metrics = importlib.import_module("3dal_pytorch_amd.metrics")
fit = importlib.import_module("3dal_pytorch_amd.fit")
ev = importlib.import_module("3dal_pytorch_amd.eval")


def median_ms(fn, iters):
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    marks[0].record()
    for i in range(iters):
        fn()
        marks[i + 1].record()
    torch.cuda.synchronize()
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(iters))
    return per[len(per) // 2]


def metric_inputs(B, N, dev):
    bp = torch.randn(B, 39, device=dev)
    out = {"center": bp[:, 0:3], "heading_scores": bp[:, 3:15], "heading_residuals": torch.randn(B, 12, device=dev),
           "size_scores": bp[:, 27:30], "size_residuals": torch.randn(B, 3, 3, device=dev),
           "logits": torch.randn(B, N, 2, device=dev)}
    lab = {"center_label": torch.randn(B, 3, device=dev), "heading_class_label": torch.randint(0, 12, (B,), device=dev),
           "heading_residuals_label": torch.randn(B, device=dev), "size_class_label": torch.randint(0, 3, (B,), device=dev),
           "size_residual_label": torch.randn(B, 3, device=dev), "mask_label": (torch.rand(B, N, device=dev) > 0.5).float()}
    return out, lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp32", choices=["fp32", "f16x3"])
    ap.add_argument("--sampler", default="numpy", choices=["numpy", "device"])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--fit-batches", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"precision": args.precision, "sampler": args.sampler, "unit": "ms"}

    for B, N in ((64, 4096), (4096, 1024)):
        out, lab = metric_inputs(B, N, dev)
        m = metrics.TrainMetrics(dev, N)
        loss = torch.zeros((), device=dev)
        for _ in range(3):
            m.update(out, lab, loss)
        res[f"metric_update_{B}x{N}"] = median_ms(lambda: m.update(out, lab, loss), 100)

    B, N = 64, 4096
    p, i, g = synth.static_crops(B, N, seed=3)
    pts = torch.from_numpy(p).to(dev).transpose(2, 1)
    init, gt = torch.from_numpy(i).to(dev), torch.from_numpy(g).to(dev)
    lab = {"mask_label": (torch.rand((B, N), device=dev) > 0.6).float(), "center_label": torch.randn((B, 3), device=dev),
           "heading_class_label": torch.randint(0, 12, (B,), device=dev),
           "heading_residuals_label": 0.1 * torch.randn((B,), device=dev),
           "size_class_label": torch.randint(0, 3, (B,), device=dev), "size_residual_label": 0.3 * torch.randn((B, 3), device=dev)}
    model = sm.StaticModelOneBoxEst()
    model.load_state_dict({k: torch.as_tensor(v) for k, v in synth.state_dict("static_one").items()})
    model = model.to(dev).train()
    model.precision, model.sampler = args.precision, args.sampler
    crit = losses.FrustumPointNetLossOneBoxEst()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    m = metrics.TrainMetrics(dev, N)

    def step(with_metric):
        o = model(pts, init, gt)
        loss = crit(o, *fit._criterion_args(lab))["total_loss"]
        opt.zero_grad()
        loss.backward()
        opt.step()
        if with_metric:
            m.update(o, lab, loss)
    np.random.seed(0)
    for _ in range(5):
        step(True)
    plain, with_m = [], []
    for _ in range(3):                                   # interleaved: drift of the box hits both alike
        plain.append(median_ms(lambda: step(False), args.iters))
        with_m.append(median_ms(lambda: step(True), args.iters))
    res["step_ms"], res["step_with_metric_ms"] = float(np.median(plain)), float(np.median(with_m))
    res["metric_share_of_step"] = res["step_with_metric_ms"] / res["step_ms"] - 1.0

    with tempfile.TemporaryDirectory() as tmp:
        n_tracks = 64 * args.fit_batches + 40
        paths = synth.segment_files(tmp, 5, n_frames=4, n_tracks=n_tracks)[0]
        infos = ev.reorganize_info(pickle.load(open(paths["infos"], "rb")))
        annos = ev.Annos(infos)
        track = ev.preprocessing(pickle.load(open(paths["static"], "rb")), annos)
        keys = list(track)[:64 * args.fit_batches]
        data = fit.StaticBatches({k: track[k] for k in keys}, annos, sampler=args.sampler, device=dev)
        fm = sm.StaticModelOneBoxEst().to(dev)
        fm.precision, fm.sampler = args.precision, args.sampler
        fopt = torch.optim.Adam(fm.parameters(), lr=1e-3, weight_decay=1e-4)
        times = []
        for e in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mt, drawn = fit.train_one_epoch(fm, data, crit, fopt, 64, N, False, item_base=e * len(keys))
            mt.result()                                  # the epoch's one read
            times.append((time.perf_counter() - t0) * 1e3 / (drawn // 64))
        res["fit_steps_per_epoch"] = len(keys) // 64
        res["fit_ms_per_step"] = float(np.median(times[1:]))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
