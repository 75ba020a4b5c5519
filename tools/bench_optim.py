#!/usr/bin/env python3
"""Measure the optimiser step (3dal_pytorch_amd/solver.py: dal3_optim_grad_norm, dal3_optim_step) and write
profiles/bench_optim.json:

    python tools/bench_optim.py [--iters 200] [--warmup 20] [--burst 50] [--out profiles/bench_optim.json]

At VoxelNet's real parameter set (the Waymo config's dimensions: VoxelFeatureExtractorV3, SpMiddleResNetFHD, RPN [5, 5] /
[128, 256], CenterHead of one 3-class task), random weights and gradients: the device step with the one-cycle table
attached and the clip at 35 armed, beside the BASELINE: the reference's formulation in stock PyTorch-ROCm ops on the same GPU
and an equal model — OneCycle's values written into the groups, one `p.data.mul_(1 - wd * lr)` per parameter,
`clip_grad_norm_(max_norm=35)`, `torch.optim.Adam.step()` (torch's default multi-tensor path).

Two clocks, both host wall clock ending in a device synchronise, the two sides alternating inside one process after every
shape is warmed: `call` is one step per synchronise (what a loop that reads the loss every iteration sees); `stream` is
--burst steps enqueued back to back per synchronise, per step (the host running ahead). Then both as a replayed hipGraph:
the device step captured as it is; the stock side with Adam(capturable=True), where it can be captured (the reason is
recorded where it cannot). Medians and spreads are recorded; no ratio is fixed in advance."""
import argparse
import copy
import functools
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

detector = importlib.import_module("3dal_pytorch_amd.detector")
sparse = importlib.import_module("3dal_pytorch_amd.sparse")
solver = importlib.import_module("3dal_pytorch_amd.solver")

WD, MAX_NORM, TOTAL_STEP = 0.01, 35.0, 1000
ONE_CYCLE = dict(lr_max=0.003, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4)


def voxelnet():
    return detector.VoxelNet(
        reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5), backbone=sparse.SpMiddleResNetFHD(num_input_features=5),
        neck=dict(type="RPN", layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[128, 256], us_layer_strides=[1, 2],
                  us_num_filters=[256, 256], num_input_features=256),
        bbox_head=dict(type="CenterHead", in_channels=512, tasks=[dict(num_class=3, class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"])],
                       dataset="waymo", weight=2, code_weights=[1.0] * 8,
                       common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2)}))


def stats(v):
    v = np.asarray(v)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "p90_ms": float(np.percentile(v, 90)), "n": int(v.size)}


def wall(fn, n=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def alternate(fns, iters, n=1):
    w = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            w[k].append(wall(fn, n))
    return {k: stats(v) for k, v in w.items()}


class Stock:
    """the reference's OptimWrapper.step over torch.optim.Adam, with the hook's clip, in stock ops"""

    def __init__(self, model, table, capturable=False):
        groups = [solver.trainable_params(g) for g in solver.split_bn_bias(solver.get_layer_groups(model))]
        self.params = groups[0] + groups[1]
        self.adam = torch.optim.Adam([{"params": g, "lr": 0} for g in groups], betas=(0.9, 0.99), amsgrad=False, capturable=capturable)
        self.table, self.t = table, 0

    def step(self):
        lr, mom = self.table[min(self.t, len(self.table) - 1)]
        self.t += 1
        for g in self.adam.param_groups:
            g["lr"], g["betas"], g["weight_decay"] = lr, (mom, g["betas"][1]), 0
        for p in self.params:
            p.data.mul_(1 - WD * lr)
        torch.nn.utils.clip_grad_norm_(self.params, max_norm=MAX_NORM, norm_type=2)
        self.adam.step()


def capture(fn, warm=3):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn()
    return g


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--burst", type=int, default=50)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_optim.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mine_model = voxelnet().to(dev).train()
    stock_model = copy.deepcopy(mine_model)
    opt = solver.OptimWrapper.create(functools.partial(torch.optim.Adam, betas=(0.9, 0.99), amsgrad=0.0), 3e-3,
                                     solver.get_layer_groups(mine_model), wd=WD, true_wd=True, bn_wd=True)
    sched = solver.OneCycle(opt, TOTAL_STEP, **ONE_CYCLE).attach()
    opt.max_norm = MAX_NORM
    stock = Stock(stock_model, sched.table(lr=ONE_CYCLE["lr_max"] / ONE_CYCLE["div_factor"], mom=ONE_CYCLE["moms"][0]))
    assert [q.shape for q in stock.params] == [q.shape for q in opt.params]
    g = torch.Generator(device=dev).manual_seed(1)
    for q, s in zip(opt.params, stock.params):
        q.grad.copy_(torch.randn(q.shape, device=dev, generator=g) * 0.05)        # a norm beyond 35: the clip binds
        s.grad = q.grad.detach().clone()
    res = {"bench": "optim", "device": torch.cuda.get_device_name(0), "model": "VoxelNet (Waymo config dimensions), random weights and gradients",
           "tensors": len(opt.params), "elements": int(sum(q.numel() for q in opt.params)), "flat_elements": opt.n_flat,
           "chunks": opt._n_chunks, "norm_partials": opt._n_partials, "iters": a.iters, "warmup": a.warmup, "burst": a.burst,
           "timing": "host wall clock ending in a device synchronise; the device step and the stock formulation alternate inside one "
                     "process; call: one step per synchronise, stream: `burst` steps per synchronise, per step",
           "baseline": "the reference's formulation in stock PyTorch-ROCm ops, same GPU, equal model: one p.data.mul_ per parameter, "
                       "clip_grad_norm_(35), torch.optim.Adam.step() (multi-tensor path)",
           "device_step_launches": 2}
    # one step each from equal states: the same update within float32
    opt.step()
    stock.step()
    torch.cuda.synchronize()
    d = max(float((q.detach() - s.detach()).abs().max()) for q, s in zip(opt.params, stock.params))
    res["first_step_max_abs_difference"] = d
    res["first_step_norm"] = float(opt.total_norm())
    fns = {"device_step": opt.step, "stock_pytorch": stock.step}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    res["call"] = alternate(fns, a.iters)
    res["stream"] = alternate(fns, max(a.iters // 10, 10), a.burst)
    res["zero_grad_and_step_call"] = alternate({"device_step": lambda: (opt.zero_grad(), opt.step()),
                                                "stock_pytorch": lambda: (stock.adam.zero_grad(set_to_none=False), stock.step())}, a.iters)
    for k in ("call", "stream"):
        res[k]["device_over_stock"] = res[k]["device_step"]["median_ms"] / res[k]["stock_pytorch"]["median_ms"]
    print(json.dumps({k: res[k] for k in ("tensors", "elements", "chunks", "call", "stream")}))

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    save()
    # replayed graphs: the device step first (a failed capture of the stock side may leave the process unusable)
    graphs = {"device_step": capture(opt.step)}
    for _ in range(a.warmup):
        graphs["device_step"].replay()
    alone = {"device_step": graphs["device_step"].replay}
    res["graph"] = {"device_step_nodes": 2, "device_step_alone_call": alternate(alone, a.iters)["device_step"],
                    "device_step_alone_stream": alternate(alone, max(a.iters // 10, 10), a.burst)["device_step"]}
    save()
    try:
        cap_model = copy.deepcopy(stock_model)
        cap = Stock(cap_model, stock.table, capturable=True)
        for q, s in zip(cap.params, stock.params):
            q.grad = s.grad.detach().clone()
        graphs["stock_pytorch"] = capture(cap.step)
        res["graph"]["stock_captured"] = True
    except Exception as e:          # recorded, not hidden: the stock side has no graph figure then
        res["graph"]["stock_captured"] = False
        res["graph"]["stock_capture_error"] = f"{type(e).__name__}: {str(e)[:300]}"
        save()
        print(json.dumps(res["graph"]))
        return
    replays = {k: g.replay for k, g in graphs.items()}
    for _ in range(a.warmup):
        for fn in replays.values():
            fn()
    res["graph"]["call"] = alternate(replays, a.iters)
    res["graph"]["stream"] = alternate(replays, max(a.iters // 10, 10), a.burst)
    res["graph"]["note"] = "the stock graph bakes the learning rate of its capture into the decay's multiplier; the device step's graph reads the table"
    for k in ("call", "stream"):
        res["graph"][k]["device_over_stock"] = res["graph"][k]["device_step"]["median_ms"] / res["graph"][k]["stock_pytorch"]["median_ms"]
    save()
    print(json.dumps(res["graph"]))


if __name__ == "__main__":
    main()
