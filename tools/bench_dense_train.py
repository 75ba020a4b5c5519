#!/usr/bin/env python3
"""Measure the training route of the detector's dense stage (rpn.py's train_forward: dal3_conv2d on the raw pack, the data
gradients through dal3_conv2d / dal3_conv2d_dgrad, the weight gradients through dal3_conv2d_wgrad) and write
profiles/bench_dense_train.json:

    python tools/bench_dense_train.py [--iters 10] [--warmup 3] [--out profiles/bench_dense_train.json]

Two shapes, in one job: the VoxelNet neck and head (a 188 x 188 map of 256 channels, B = 1 and 4) and the PointPillars ones
(468 x 468, 64 channels, B = 1), seeded weights, a canvas with about 30 % of its cells occupied.

Per layer class (form, stride, widths and map size; `count` layers of the network share it) it records the time of the
forward convolution (the yardstick of the backward), of the data gradient as _Conv2dFunction runs it (the pack of the
transposed weight, or dal3_conv2d_dgrad_pack, included) and of the weight gradient with its bias sum, HIP events around
the enqueued launches, the median of --iters runs after --warmup; the algorithmic multiply-accumulates (dgrad and wgrad
each execute the forward's, so backward over forward is 2.0 by the algorithm) and the workspace bytes of the weight
gradient. Then `train_forward` + `backward()` of neck + head, BatchNorm in train mode, beside `composite()` + `backward()`
(stock torch ops and stock autograd: the training path before these kernels) on the same GPU in the same job, the two
routes alternating, wall clock between two synchronisations, the median.

No time is fixed in advance: the ratio to the composite route is reported whichever way it falls."""
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
import rpn_ref as R  # noqa: E402

hip = importlib.import_module("3dal_pytorch_amd._hip")
rpn = importlib.import_module("3dal_pytorch_amd.rpn")
PEAK_TFLOPS = 157.3                             # fp32 MFMA: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz
TASKS = [dict(num_class=3, class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"])]
COMMON = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2)}
SHAPES = {
    "voxelnet": dict(size=188, batches=(1, 4),
                     neck=dict(layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[128, 256], us_layer_strides=[1, 2],
                               us_num_filters=[256, 256], num_input_features=256),
                     head=dict(in_channels=512, tasks=TASKS, dataset="waymo", weight=2, code_weights=[1.0] * 8, common_heads=COMMON)),
    "pointpillars": dict(size=468, batches=(1,), neck=R.NECK, head=R.HEAD),
}


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def layer_classes(neck, head, B, size):
    """every convolution of neck + head at a (size, size) canvas -> {(kind, stride, c_in, c_out, H, W): count}, in forward order"""
    classes = {}

    def walk(seq, h, w):
        for conv, _, _ in rpn._split(seq):
            kind, stride = rpn.layer_kind(conv)
            key = (kind, stride, conv.in_channels, conv.out_channels, h, w)
            classes[key] = classes.get(key, 0) + 1
            h, w = rpn.out_size(kind, stride, h, w)
        return h, w

    h, w = size, size
    for i, block in enumerate(neck.blocks):
        h, w = walk(block, h, w)
        if i - neck._upsample_start_idx >= 0:
            oh, ow = walk(neck.deblocks[i - neck._upsample_start_idx], h, w)
    for seq in head._sequences():
        walk(seq, oh, ow)
    return classes


def measure_class(key, B, a, dev):
    kind, stride, c_in, c_out, H, W = key
    deconv = kind in (hip.CONV2D_DECONV2, hip.CONV2D_DECONV4)
    k = 3 if kind == hip.CONV2D_3X3 else 1 if kind == hip.CONV2D_1X1 else stride
    g = torch.Generator(device="cpu").manual_seed(1)
    w = (torch.randn((c_in, c_out, k, k) if deconv else (c_out, c_in, k, k), generator=g) * (2.0 / (c_in * k * k)) ** 0.5).to(dev)
    bias = torch.zeros(c_out, device=dev)
    x = torch.rand((B, c_in, H, W), generator=g).to(dev)
    OH, OW = rpn.out_size(kind, stride, H, W)
    dy = torch.randn((B, c_out, OH, OW), generator=g).to(dev)
    packed = rpn.pack_raw(w, bias, kind, c_in, c_out)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    with torch.no_grad():
        ms_f = timed(lambda: rpn.conv2d(x, packed, kind, stride, False, c_out, out=y), a.iters, a.warmup)
        ms_d = timed(lambda: rpn.conv2d_dgrad(dy, w, kind, stride, (H, W), out=dx), a.iters, a.warmup)
        ms_w = timed(lambda: rpn.conv2d_wgrad(x, dy, kind, stride, w.shape), a.iters, a.warmup)
    taps = 9 if kind == hip.CONV2D_3X3 else 1 if kind == hip.CONV2D_1X1 else stride * stride
    ph, pw = (H, W) if deconv else (OH, OW)
    macs = B * ph * pw * c_in * c_out * taps
    rate = lambda ms: 2 * macs / (ms * 1e-3) / 1e12 / PEAK_TFLOPS
    return {"kind": {hip.CONV2D_3X3: "3x3", hip.CONV2D_1X1: "1x1"}.get(kind, "deconv"), "stride": stride, "c_in": c_in, "c_out": c_out,
            "H": H, "W": W, "macs": macs, "forward_ms": ms_f, "dgrad_ms": ms_d, "wgrad_ms": ms_w,
            "forward_share_of_peak": rate(ms_f), "dgrad_share_of_peak": rate(ms_d), "wgrad_share_of_peak": rate(ms_w),
            "backward_over_forward": (ms_d + ms_w) / ms_f,
            "wgrad_workspace_bytes": int(rpn.conv2d_wgrad_workspace_bytes(kind, stride, c_in, c_out, B, H, W))}


def step(neck, head, x, route):
    for m in (neck, head):
        m.zero_grad(set_to_none=True)
    n = neck.train_forward(x) if route == "hip" else neck.composite(x)
    preds = head.train_forward(n) if route == "hip" else head.composite(n)
    sum(v.sum() for d in preds for v in d.values()).backward()


def measure(name, B, a, dev):
    cfg = SHAPES[name]
    torch.manual_seed(0)
    neck, head = rpn.RPN(**cfg["neck"]).to(dev).train(), rpn.CenterHead(**cfg["head"]).to(dev).train()
    assert neck.hip_serves() and head.hip_serves()
    size, c = cfg["size"], cfg["neck"]["num_input_features"]
    g = torch.Generator(device="cpu").manual_seed(2)
    x = (torch.rand((B, c, size, size), generator=g) * 2.0 * (torch.rand((B, 1, size, size), generator=g) < 0.3)).to(dev).requires_grad_()
    row = {"shape": name, "B": B, "size": size, "channels_in": c, "classes": []}
    tot = {"forward_ms": 0.0, "dgrad_ms": 0.0, "wgrad_ms": 0.0}
    for key, count in layer_classes(neck, head, B, size).items():
        r = dict(measure_class(key, B, a, dev), count=count)
        row["classes"].append(r)
        for k in tot:
            tot[k] += count * r[k]
        print(json.dumps(r), flush=True)
    row.update(tot, backward_over_forward=(tot["dgrad_ms"] + tot["wgrad_ms"]) / tot["forward_ms"], algorithmic_backward_over_forward=2.0,
               wgrad_workspace_bytes_max=max(r["wgrad_workspace_bytes"] for r in row["classes"]))
    wall = {"hip": [], "composite": []}
    for i in range(a.warmup + a.iters):
        for route in ("hip", "composite") if i % 2 == 0 else ("composite", "hip"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(neck, head, x, route)
            torch.cuda.synchronize()
            if i >= a.warmup:
                wall[route].append((time.perf_counter() - t0) * 1e3)
    row["train_forward_backward_ms"] = float(np.median(wall["hip"]))
    row["composite_backward_ms"] = float(np.median(wall["composite"]))
    row["hip_over_composite"] = row["train_forward_backward_ms"] / row["composite_backward_ms"]
    row["spread_ms"] = {k: [float(np.min(v)), float(np.max(v))] for k, v in wall.items()}
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", nargs="+", default=list(SHAPES))
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_dense_train.json"))
    a = p.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "dense_train", "device": torch.cuda.get_device_name(0), "peak_tflops": PEAK_TFLOPS, "iters": a.iters,
           "warmup": a.warmup, "wgrad_slice": hip.CONV2D_WGRAD_SLICE,
           "baseline": "composite() + backward(): stock torch ops and stock autograd, same GPU, same job, routes alternating",
           "canvas": "synthetic: about 30 % of the cells occupied, seeded weights", "rows": []}
    for name in a.shapes:
        for B in SHAPES[name]["batches"]:
            res["rows"].append(measure(name, B, a, dev))
            print(json.dumps({k: v for k, v in res["rows"][-1].items() if k != "classes"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(compact(res))


def compact(res):
    """the result as JSON with one line per layer class and per shape, floats at four significant digits"""
    def sig(v):
        if isinstance(v, float):
            return float(f"{v:.4g}")
        if isinstance(v, dict):
            return {k: sig(x) for k, x in v.items()}
        return [sig(x) for x in v] if isinstance(v, (list, tuple)) else v

    rows = []
    for row in res["rows"]:
        head = json.dumps(sig({k: v for k, v in row.items() if k != "classes"}))
        classes = ",\n".join("   " + json.dumps(sig(c)) for c in row["classes"])
        rows.append('  %s, "classes": [\n%s]}' % (head[:-1], classes))
    top = json.dumps({k: v for k, v in res.items() if k != "rows"})
    return '%s, "rows": [\n%s\n]}\n' % (top[:-1], ",\n".join(rows))


if __name__ == "__main__":
    main()
