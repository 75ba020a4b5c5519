#!/usr/bin/env python3
"""The detector's dense stage — RPN neck + CenterHead of the PointPillars configuration — at the size of a Waymo frame:
a 468 x 468 canvas of 64 channels with about 30 % of its cells occupied, batch sizes --batches, on seeded weights
(tests/rpn_ref.py). Times on the current GPU, with device events around windows of at least --window seconds that
alternate between the two routes after both were warmed on the shape:
  hip        the eval-mode forward: dal3_conv2d for every layer (include/dal3.h)
  composite  the only route there was before: `composite()`, the reference formulation through stock PyTorch-ROCm
             convolutions, BatchNorms and ReLUs on the same GPU
and records beside them the algorithmic FLOP (2 x MACs from the shapes, `flop` below), the FLOP the kernel's tiles execute
(32 GEMM rows, 8 x 32 pixels, 8 input channels), the share of the 157.3 TF fp32-MFMA peak, the largest difference between
the two routes' outputs, and the compiler's register / scratch / LDS counts of every kernel. One JSON line; --out writes it
to a file (after every batch size, so that an interrupted run leaves what it measured).
    python tools/bench_detector.py [--batches 1 4 --window 1.0 --out profiles/bench_detector.json]
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
rpn = importlib.import_module("3dal_pytorch_amd.rpn")

PEAK_TFLOPS = 157.3                             # fp32 MFMA: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz
SIZE = 468


def flop(neck, head, H, W, B=1):
    """(algorithmic, executed) FLOP of neck + head on a (B, C, H, W) canvas, layer by layer from the modules' own plans"""
    algo = executed = 0

    def add(plan_row, h, w):
        nonlocal algo, executed
        conv, _, kind, stride, _ = plan_row
        a, e = rpn.conv2d_flop(kind, stride, conv.in_channels, conv.out_channels, h, w, B)
        algo, executed = algo + a, executed + e
        return rpn.out_size(kind, stride, h, w)

    plan, at, h, w = neck._plan(), 0, H, W
    n_block_layers = sum(len(rpn._split(b)) for b in neck.blocks)
    for i, block in enumerate(neck.blocks):
        for _ in rpn._split(block):
            h, w = add(plan[at], h, w)
            at += 1
        if i - neck._upsample_start_idx >= 0:
            add(plan[n_block_layers + i - neck._upsample_start_idx], h, w)
    for row in head._plan():
        add(row, H, W)                          # every layer of the head runs at the canvas's size
    return algo, executed


def window(fn, seconds):
    """calls of fn for at least `seconds` between two device events -> (ms per call, calls)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, t0 = 0, time.perf_counter()
    a.record()
    while True:
        fn()
        n += 1
        if n % 4 == 0 or n == 1:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n, n


def kernel_resources():
    """registers, scratch and LDS of every kernel of csrc/dal3_conv2d.hip from the compiler's own remarks, or None"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(ROOT, "3dal_pytorch_amd", "csrc", "dal3_conv2d.hip")
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
            m2 = re.search(r"\d+([a-z0-9_]+_kernel)(?:ILi(\d)ELi(\d)ELb([01])ELi(\d)E)?", m.group(1))
            cur = (m2.group(1) + (f"<{m2.group(2)},{m2.group(3)},{m2.group(4)},{m2.group(5)}>" if m2.group(2) else "")) if m2 else m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]+\])?): (\d+)", line)
        if m and cur and m.group(1).strip() in keys:
            out[cur][keys[m.group(1).strip()]] = int(m.group(2))
    return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--size", type=int, default=SIZE)
    ap.add_argument("--skip_composite", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rpn_ref as R
    dev = torch.device("cuda")
    neck, head = rpn.RPN(**R.NECK), rpn.CenterHead(**R.HEAD)
    neck.load_state_dict({k: torch.as_tensor(v) for k, v in R.neck_weights().items()}, strict=True)
    head.load_state_dict({k: torch.as_tensor(v) for k, v in R.head_weights().items()}, strict=True)
    neck, head = neck.to(dev).eval(), head.to(dev).eval()
    res = {"bench": "detector", "size": a.size, "device": torch.cuda.get_device_name(0), "peak_tflops": PEAK_TFLOPS,
           "window_s": a.window, "kernel_resources": kernel_resources(), "batches": {}}

    def hip_route(x):
        return head(neck(x))

    def composite_route(x):
        return head.composite(neck.composite(x))

    for B in a.batches:
        x = torch.from_numpy(R.canvas(f"bench{B}", (B, 64, a.size, a.size))).to(dev)
        algo, executed = flop(neck, head, a.size, a.size, B)
        row = {"algorithmic_flop": algo, "executed_flop": executed, "occupied": float((x != 0).any(1).float().mean())}
        with torch.no_grad():
            got = hip_route(x)                  # warm
            hip_route(x)
            if not a.skip_composite:
                want = composite_route(x)
                composite_route(x)
                row["max_abs_diff"] = max(float((got[0][k] - want[0][k]).abs().max()) for k in got[0])
                row["max_abs_value"] = max(float(want[0][k].abs().max()) for k in want[0])
            torch.cuda.synchronize()
            hip_ms, comp_ms = [], []
            for _ in range(a.windows):
                hip_ms.append(window(lambda: hip_route(x), a.window))
                if not a.skip_composite:
                    comp_ms.append(window(lambda: composite_route(x), a.window))
        row["hip_ms"] = float(np.median([t for t, _ in hip_ms]))
        row["hip_windows"] = [[round(t, 3), n] for t, n in hip_ms]
        row["hip_algorithmic_tflops"] = algo / (row["hip_ms"] * 1e-3) / 1e12
        row["hip_executed_tflops"] = executed / (row["hip_ms"] * 1e-3) / 1e12
        row["hip_share_of_peak"] = row["hip_algorithmic_tflops"] / PEAK_TFLOPS
        row["hip_executed_share_of_peak"] = row["hip_executed_tflops"] / PEAK_TFLOPS
        if comp_ms:
            row["composite_ms"] = float(np.median([t for t, _ in comp_ms]))
            row["composite_windows"] = [[round(t, 3), n] for t, n in comp_ms]
            row["composite_algorithmic_tflops"] = algo / (row["composite_ms"] * 1e-3) / 1e12
            row["hip_over_composite_time"] = row["hip_ms"] / row["composite_ms"]
        res["batches"][str(B)] = row
        print(f"B={B}: {json.dumps(row)}", file=sys.stderr, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
