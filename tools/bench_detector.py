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

--precision fp16 | bf16 (default fp32: everything above, unchanged) times three routes in one job instead, alternating:
  hip_fp32        the fp32 kernel route (dal3_conv2d)
  hip_<precision> the same modules with `precision` set: dal3_conv2d_lp on 16-bit MFMA operands, float32 maps
  half_composite  `composite()` of .half() copies on a .half() canvas: stock PyTorch-ROCm half-precision convolutions
and records the ratios, the 16-bit kernel's executed FLOP (16 input channels a k-step), the compiler's resources of
csrc/dal3_conv2d_lp.hip, the output difference of the two kernel routes, and for the seeded sweep of --double-flip
(`PointPillars.detect`, --points points) how many kept boxes differ between "fp32" and the 16-bit precision.
    python tools/bench_detector.py --precision fp16 --out profiles/bench_detector_lp.json

--double-flip measures the test-time augmentation instead (profiles/bench_tta.json): `PointPillars.detect` on one seeded
sweep of --points points over the same 468 x 468 grid, with and without test_cfg.double_flip, and the merge of the four
views alone two ways on the head's own outputs:
  fused      DoubleFlipPost.decode: dal3_center_decode_flip4 reads the four views' NCHW channel slices and writes rows
  composite  the reference's formulation in stock PyTorch-ROCm ops (permute + contiguous, three flips written back in
             place, sigmoid / exp, the sign and 1 - x rules, six means), then logit / log of the merged hm / dim so that
             the existing dal3_center_decode can take the merged maps through NHWC views
    python tools/bench_detector.py --double-flip --out profiles/bench_tta.json
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


def flop(neck, head, H, W, B=1, layer_flop=None):
    """(algorithmic, executed) FLOP of neck + head on a (B, C, H, W) canvas, layer by layer from the modules' own plans;
    layer_flop: rpn.conv2d_flop (the default) or rpn.conv2d_lp_flop"""
    algo = executed = 0
    layer_flop = layer_flop or rpn.conv2d_flop

    def add(plan_row, h, w):
        nonlocal algo, executed
        conv, _, kind, stride, _ = plan_row
        a, e = layer_flop(kind, stride, conv.in_channels, conv.out_channels, h, w, B)
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


def kernel_resources(source="dal3_conv2d.hip"):
    """registers, scratch and LDS of every kernel of csrc/<source> from the compiler's own remarks, or None"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(ROOT, "3dal_pytorch_amd", "csrc", source)
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
            m2 = re.search(r"\d+([a-z0-9_]+_kernel)(?:I(?:\d([A-Z0-9]+?))?(?:Li(\d)ELi(\d)ELb([01])ELi(\d)E)?E)?", m.group(1))
            args = [g for g in (m2.groups()[1:] if m2 else ()) if g is not None]
            cur = (m2.group(1) + (f"<{','.join(args)}>" if args else "")) if m2 else m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]+\])?): (\d+)", line)
        if m and cur and m.group(1).strip() in keys:
            out[cur][keys[m.group(1).strip()]] = int(m.group(2))
    return out or None


TTA_VOXEL, TTA_RANGE = (0.32, 0.32, 6.0), (-74.88, -74.88, -2.0, 74.88, 74.88, 4.0)      # 468 x 468 pillars
TTA_CFG = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0],
               nms=dict(nms_pre_max_size=4096, nms_post_max_size=500, nms_iou_threshold=0.7), score_threshold=0.1,
               pc_range=[TTA_RANGE[0], TTA_RANGE[1]], out_size_factor=1, voxel_size=[0.32, 0.32])


def composite_merge(preds_dicts):
    """center_head.py:311-414's merge of the four views in stock ops -> NHWC maps of the merged samples that
    dal3_center_decode reproduces the merged values from (hm as the logit of the mean score, dim as the log of the mean)"""
    out = []
    for pd in preds_dicts:
        m = {}
        for k, v in pd.items():
            v = v.permute(0, 2, 3, 1).contiguous()
            _, H, W, C = v.shape
            v = v.reshape(-1, 4, H, W, C)
            v[:, 1] = torch.flip(v[:, 1], dims=[1])
            v[:, 2] = torch.flip(v[:, 2], dims=[2])
            v[:, 3] = torch.flip(v[:, 3], dims=[1, 2])
            m[k] = v
        hm = torch.sigmoid(m["hm"]).mean(dim=1)
        dim = torch.exp(m["dim"]).mean(dim=1)
        reg = m["reg"]
        reg[:, 1, ..., 1] = 1 - reg[:, 1, ..., 1]
        reg[:, 2, ..., 0] = 1 - reg[:, 2, ..., 0]
        reg[:, 3] = 1 - reg[:, 3]
        rot = m["rot"]
        rot[:, 1, ..., 1] *= -1
        rot[:, 2, ..., 0] *= -1
        rot[:, 3] *= -1
        d = {"hm": torch.logit(hm), "dim": torch.log(dim), "reg": reg.mean(dim=1), "height": m["height"].mean(dim=1),
             "rot": rot.mean(dim=1)}
        if "vel" in m:
            vel = m["vel"]
            vel[:, 1, ..., 1] *= -1
            vel[:, 2, ..., 0] *= -1
            vel[:, 3] *= -1
            d["vel"] = vel.mean(dim=1)
        out.append(d)
    return out


def sweep_model_and_points(n, dev):
    """the seeded PointPillars detector over the 468 x 468 grid and the seeded sweep of n points -> (model, points, offsets)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pillars_ref as P
    import rpn_ref as R
    detector = importlib.import_module("3dal_pytorch_amd.detector")
    model = detector.PointPillars(
        reader=dict(type="PillarFeatureNet", num_filters=[64, 64], num_input_features=5, with_distance=False,
                    voxel_size=TTA_VOXEL, pc_range=TTA_RANGE),
        backbone=dict(type="PointPillarsScatter", ds_factor=1), neck=dict(type="RPN", **R.NECK),
        bbox_head=dict(type="CenterHead", **R.HEAD), test_cfg=TTA_CFG, max_points=20, max_voxels=60000)
    sd = {"reader." + k: v for k, v in P.reader_weights(2, 5).items()}
    sd.update({"neck." + k: v for k, v in R.neck_weights().items()})
    sd.update({"bbox_head." + k: v for k, v in R.head_weights().items()})
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    rng = np.random.default_rng(0)
    pts = np.concatenate([np.clip(rng.normal(0, 30, (n, 2)), -74.8, 74.8), rng.uniform(-2, 4, (n, 1)), rng.uniform(0, 1, (n, 2))],
                         1).astype(np.float32)
    return model.to(dev).eval(), torch.from_numpy(pts).to(dev), np.asarray([0, n], np.int64)


def kept_boxes_that_differ(a, dev):
    """`detect` on the seeded sweep with "fp32" and with a.precision: a kept box of one run has a partner in the other when
    a box of the same label lies within one pillar (0.32 m) of its centre -> the counts (a record, not a bar)"""
    model, dpts, off = sweep_model_and_points(a.points, dev)
    with torch.no_grad():
        want = model.detect(dpts, off)[0]
        model.precision = a.precision
        got = model.detect(dpts, off)[0]

    def unmatched(p, q):
        if not p["scores"].numel() or not q["scores"].numel():
            return int(p["scores"].numel())
        d = torch.cdist(p["box3d_lidar"][:, :2].double(), q["box3d_lidar"][:, :2].double())
        d[p["label_preds"][:, None] != q["label_preds"][None, :]] = float("inf")
        return int((d.min(1).values > 0.32).sum())

    return {"points": a.points, "kept_fp32": int(want["scores"].numel()), f"kept_{a.precision}": int(got["scores"].numel()),
            f"{a.precision}_without_fp32_partner": unmatched(got, want), f"fp32_without_{a.precision}_partner": unmatched(want, got)}


def lp_bench(a):
    """--precision fp16 | bf16: see the module's docstring"""
    import copy
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rpn_ref as R
    dev, prec = torch.device("cuda"), a.precision
    neck, head = rpn.RPN(**R.NECK), rpn.CenterHead(**R.HEAD)
    neck.load_state_dict({k: torch.as_tensor(v) for k, v in R.neck_weights().items()}, strict=True)
    head.load_state_dict({k: torch.as_tensor(v) for k, v in R.head_weights().items()}, strict=True)
    neck, head = neck.to(dev).eval(), head.to(dev).eval()
    neck16, head16 = copy.deepcopy(neck), copy.deepcopy(head)
    neck16.precision = head16.precision = prec
    neck_h, head_h = copy.deepcopy(neck).half(), copy.deepcopy(head).half()
    res = {"bench": "detector_lp", "precision": prec, "size": a.size, "device": torch.cuda.get_device_name(0), "window_s": a.window,
           "kernel_resources": kernel_resources("dal3_conv2d_lp.hip"), "batches": {}}
    routes = {"hip_fp32": lambda x, xh: head(neck(x)), f"hip_{prec}": lambda x, xh: head16(neck16(x)),
              "half_composite": lambda x, xh: head_h.composite(neck_h.composite(xh))}
    for B in a.batches:
        x = torch.from_numpy(R.canvas(f"bench{B}", (B, 64, a.size, a.size))).to(dev)
        xh = x.half()
        algo, executed = flop(neck, head, a.size, a.size, B, rpn.conv2d_lp_flop)
        row = {"algorithmic_flop": algo, "executed_flop": executed, "occupied": float((x != 0).any(1).float().mean())}
        with torch.no_grad():
            outs = {k: fn(x, xh) for k, fn in routes.items()}               # warm, twice
            for fn in routes.values():
                fn(x, xh)
            want, scale = outs["hip_fp32"][0], max(float(v.abs().max()) for v in outs["hip_fp32"][0].values())
            row["max_abs_value"] = scale
            for k in (f"hip_{prec}", "half_composite"):
                row[f"{k}_max_abs_diff_to_fp32"] = max(float((outs[k][0][h].float() - want[h]).abs().max()) for h in want)
            del outs
            torch.cuda.synchronize()
            times = {k: [] for k in routes}
            for _ in range(a.windows):
                for k, fn in routes.items():
                    times[k].append(window(lambda: fn(x, xh), a.window))
        for k, w in times.items():
            row[f"{k}_ms"] = float(np.median([t for t, _ in w]))
            row[f"{k}_windows"] = [[round(t, 3), n] for t, n in w]
        row[f"hip_{prec}_algorithmic_tflops"] = algo / (row[f"hip_{prec}_ms"] * 1e-3) / 1e12
        row[f"hip_{prec}_over_hip_fp32_time"] = row[f"hip_{prec}_ms"] / row["hip_fp32_ms"]
        row[f"hip_{prec}_over_half_composite_time"] = row[f"hip_{prec}_ms"] / row["half_composite_ms"]
        res["batches"][str(B)] = row
        print(f"B={B}: {json.dumps(row)}", file=sys.stderr, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    del x, xh
    res["kept_boxes"] = kept_boxes_that_differ(a, dev)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


def double_flip_bench(a):
    """--double-flip: see the module's docstring"""
    detect = importlib.import_module("3dal_pytorch_amd.detect")
    pillars = importlib.import_module("3dal_pytorch_amd.pillars")
    dev, n = torch.device("cuda"), a.points
    model, dpts, off = sweep_model_and_points(n, dev)
    off_dev = torch.from_numpy(off).to(dev)
    flip_cfg = dict(TTA_CFG, double_flip=True)
    res = {"bench": "double_flip", "size": a.size, "points": n, "device": torch.cuda.get_device_name(0), "window_s": a.window}

    def run_detect(cfg):
        model.test_cfg = cfg
        return model.detect(dpts, off, point_offsets_device=off_dev)

    with torch.no_grad():
        plain, flipped = run_detect(TTA_CFG), run_detect(flip_cfg)
        res["occupied"] = float(model.last.voxel_offsets[1]) / (a.size * a.size)
        res["kept_plain"], res["kept_double_flip"] = int(plain[0]["scores"].numel()), int(flipped[0]["scores"].numel())
        # the head's outputs of the four views, for the merge alone
        r = pillars.voxelize(*pillars.double_flip(dpts, off, off_dev)[:2], TTA_VOXEL, TTA_RANGE, 20, 60000)
        canvas = model.reader.forward_canvas(r.voxels, r.num_points, r.coordinates, 4, [a.size, a.size], n_pillars=r.n_pillars)
        preds = model.bbox_head(model.neck(canvas))
        fused_post = detect.DoubleFlipPost(flip_cfg, model.bbox_head.num_classes)
        plain_post = detect.CenterHeadPost(TTA_CFG, model.bbox_head.num_classes)

        def fused():
            return fused_post.decode(preds)

        def composite():
            return plain_post.decode(composite_merge(preds), layout="NHWC")

        x, y = fused(), composite()
        res["candidates_fused"], res["candidates_composite"] = x["seg_count"].cpu().tolist(), y["seg_count"].cpu().tolist()
        torch.cuda.synchronize()
        rows = {"detect_ms": lambda: run_detect(TTA_CFG), "detect_double_flip_ms": lambda: run_detect(flip_cfg),
                "merge_fused_ms": fused, "merge_composite_ms": composite}
        times = {k: [] for k in rows}
        for _ in range(a.windows):
            for k, fn in rows.items():
                times[k].append(window(fn, a.window))
    for k, w in times.items():
        res[k] = float(np.median([t for t, _ in w]))
        res[k.replace("_ms", "_windows")] = [[round(t, 3), c] for t, c in w]
    res["double_flip_over_plain"] = res["detect_double_flip_ms"] / res["detect_ms"]
    res["fused_over_composite_time"] = res["merge_fused_ms"] / res["merge_composite_ms"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--size", type=int, default=SIZE)
    ap.add_argument("--skip_composite", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--double-flip", action="store_true", help="time the test-time augmentation instead (see above)")
    ap.add_argument("--points", type=int, default=180000, help="points of the --double-flip sweep")
    ap.add_argument("--precision", choices=["fp32", "fp16", "bf16"], default="fp32",
                    help="fp16 / bf16: time the fp32 kernels, the 16-bit kernels and stock half convolutions in one job (see above)")
    a = ap.parse_args()
    if a.double_flip:
        return double_flip_bench(a)
    if a.precision != "fp32":
        a.out = a.out or os.path.join(ROOT, "profiles", "bench_detector_lp.json")
        return lp_bench(a)
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
