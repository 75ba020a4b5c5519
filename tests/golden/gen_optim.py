#!/usr/bin/env python3
"""Generate tests/golden/optim.npz from the REAL reference (jacky121298/3DAL_PyTorch): its own `OptimWrapper`
(det3d/solver/fastai_optim.py) over torch.optim.Adam, its `OneCycle`, `ExponentialDecay` and `ManualStepping`
(det3d/solver/learning_schedules_fastai.py) and torch's `clip_grad_norm_`, in the order of OptimizerHook.after_train_iter, on
the seeded model and gradients of tests/solver_ref.py.

Run only where the reference checkout exists (DAL3_REFERENCE, as tests/golden/gen_pillars.py reads it), on the CPU:
    python tests/golden/gen_optim.py

The two solver files are loaded by path at run time (`collections.Iterable` is given back to them first); `flatten_model`
and `get_layer_groups` are the reference's own function definitions, compiled out of det3d/torchie/apis/train.py's syntax tree
without importing that module (its import chain needs the whole detector). Nothing of the reference is copied here.

What is recorded: see tests/solver_ref.py. Every run is made twice, in float32 and with the model in .double(); the
.double() run is the truth. Asserted here: a third of the steps clip (norms of about 520 and about 16 against 35), the
restatement of tests/solver_ref.py reproduces the float64 run, and OneCycle(total_step=1) is refused by the reference's own
assertion (recorded as `sched_1_raises`). Fixed timestamps: a rerun reproduces the archive byte for byte."""
import ast
import collections
import collections.abc
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gen_pillars as G  # noqa: E402
import solver_ref as T  # noqa: E402


def import_reference():
    collections.Iterable = collections.abc.Iterable
    opt = G._load_file("ref_fastai_optim", "det3d/solver/fastai_optim.py")
    sched = G._load_file("ref_learning_schedules", "det3d/solver/learning_schedules_fastai.py")
    tree = ast.parse(open(os.path.join(G.REF, "det3d/torchie/apis/train.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("flatten_model", "get_layer_groups")]
    assert len(keep) == 2
    ns = {"nn": torch.nn}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "train.py", "exec"), ns)
    return opt, sched, ns["get_layer_groups"]


def schedule(sched_mod, make, n):
    fake = sched_mod.FakeOptim()
    s = make(fake, n)
    out = np.zeros((n, 2), np.float64)
    for i in range(n):
        s.step(i)
        out[i] = fake.lr, fake.mom
    return out


def run_reference(opt_mod, sched_mod, get_layer_groups, config, init, names, grad_fn, double):
    true_wd, bn_wd = T.CONFIGS[config]
    model = T.build_model(init, names)
    if double:
        model = model.double()
    opt = opt_mod.OptimWrapper.create(partial(torch.optim.Adam, betas=T.ADAM["betas"], amsgrad=0.0), T.LR0, get_layer_groups(model),
                                      wd=T.WD, true_wd=true_wd, bn_wd=bn_wd)
    sched = sched_mod.OneCycle(opt, T.TOTAL_STEP, T.ONE_CYCLE["lr_max"], T.ONE_CYCLE["moms"], T.ONE_CYCLE["div_factor"],
                               T.ONE_CYCLE["pct_start"])
    params = [p for g in opt.opt.param_groups for p in g["params"]]
    by_id = {id(p): n for n, p in model.named_parameters()}
    order = [by_id[id(p)] for p in params]
    n_bn = len(opt.opt.param_groups[1]["params"])
    sizes = [p.numel() for p in params]
    off = T.offsets(sizes)
    out = []
    for t in range(T.STEPS):
        sched.step(t)
        opt.zero_grad()
        g = grad_fn(t)
        for i, p in enumerate(params):
            p.grad = torch.from_numpy(g[off[i]:off[i + 1]].copy()).to(p.dtype).view(p.shape)
        norm = torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.requires_grad], max_norm=T.MAX_NORM, norm_type=2)
        opt.step()
        st = opt.opt.state
        out.append(dict(norm=float(norm), lr=float(opt.lr), mom=float(opt.mom), p=T.flat(params),
                        m=T.flat([st[p]["exp_avg"] for p in params]), v=T.flat([st[p]["exp_avg_sq"] for p in params])))
        assert all(int(st[p]["step"]) == t + 1 for p in params)
    frozen = dict(model.named_parameters())["frozen.weight"]
    assert np.array_equal(frozen.detach().numpy(), T.build_model(init, names).frozen.weight.detach().numpy())
    return order, sizes, n_bn, out


def main():
    torch.set_num_threads(1)
    opt_mod, sched_mod, get_layer_groups = import_reference()
    out = {}
    # the parameter order, from the reference's own groups over the seeded model
    model = T.build_model()
    T.seeded_init(model)
    probe = opt_mod.OptimWrapper.create(partial(torch.optim.Adam, betas=T.ADAM["betas"], amsgrad=0.0), T.LR0, get_layer_groups(model),
                                        wd=T.WD, true_wd=True, bn_wd=True)
    by_id = {id(p): n for n, p in model.named_parameters()}
    names = [by_id[id(p)] for g in probe.opt.param_groups for p in g["params"]]
    named = dict(model.named_parameters())
    init = T.flat([named[n] for n in names]).astype(np.float32)
    q, scale = T.seeded_grads(len(init))
    out.update(names=np.array(names), init=init, grad_q=q, grad_scale=scale)
    grad_fn = lambda t: T.grads_of(out, t)

    for c in T.CONFIGS:
        order, sizes, n_bn, r32 = run_reference(opt_mod, sched_mod, get_layer_groups, c, init, names, grad_fn, False)
        order64, _, _, r64 = run_reference(opt_mod, sched_mod, get_layer_groups, c, init, names, grad_fn, True)
        assert order == names == order64
        out["sizes"], out["n_bn"] = np.array(sizes, np.int64), np.int64(n_bn)
        norms = np.array([r["norm"] for r in r64])
        clipped = norms > T.MAX_NORM
        assert clipped.sum() * 3 == T.STEPS and norms[clipped].min() > 500 and norms[~clipped].max() < 17, norms
        out[f"{c}/norm64"], out[f"{c}/norm32"] = norms, np.array([r["norm"] for r in r32])
        out[f"{c}/lr"], out[f"{c}/mom"] = np.array([r["lr"] for r in r64]), np.array([r["mom"] for r in r64])
        assert np.array_equal(out[f"{c}/lr"], [r["lr"] for r in r32])
        s = np.stack([np.stack([T.sums(r[k], sizes) for k in "pmv"], 1) for r in r64])       # (steps, tensors, 3, 2)
        out[f"{c}/sum64"], out[f"{c}/sumsq64"] = s[..., 0], s[..., 1]
        # the restatement reproduces the float64 run, element by element at every step
        mine = T.run(c, init, sizes, n_bn, grad_fn, torch.float64)
        for t in range(T.STEPS):
            for k in "pmv":
                np.testing.assert_allclose(mine[t][k], r64[t][k], rtol=1e-12, atol=1e-300)
            assert abs(mine[t]["norm"] - r64[t]["norm"]) <= 1e-12 * r64[t]["norm"] and mine[t]["lr"] == r64[t]["lr"] and mine[t]["mom"] == r64[t]["mom"]
        bn0 = T.offsets(sizes)[len(sizes) - n_bn]
        keep = {"tt": ("pmv", 0), "tf": ("p", bn0), "cp": ("p", 0)}[c]
        for k in keep[0]:
            x32 = r32[-1][k][keep[1]:].astype(np.float32)
            out[f"{c}/{k}32"], out[f"{c}/{k}_d"] = x32, (r64[-1][k][keep[1]:] - x32.astype(np.float64)).astype(np.float32)
        if c == "tf":       # what is not stored of tf equals tt
            tt = run_reference(opt_mod, sched_mod, get_layer_groups, "tt", init, names, grad_fn, True)[3]
            assert np.array_equal(tt[-1]["p"][:bn0], r64[-1]["p"][:bn0]) and all(np.array_equal(tt[-1][k], r64[-1][k]) for k in "mv")

    # the schedules
    oc = lambda o, n: sched_mod.OneCycle(o, n, T.ONE_CYCLE["lr_max"], T.ONE_CYCLE["moms"], T.ONE_CYCLE["div_factor"], T.ONE_CYCLE["pct_start"])
    for n in T.SCHEDULE_STEPS:
        try:
            out[f"sched/{n}"] = schedule(sched_mod, oc, n)
        except AssertionError:
            assert n == 1
            out["sched_1_raises"] = np.bool_(True)
    out["sched_exp"] = schedule(sched_mod, lambda o, n: sched_mod.ExponentialDecay(o, n, 3e-4, 0.1, 0.8, staircase=True), 100)
    out["sched_manual"] = schedule(sched_mod, lambda o, n: sched_mod.ManualStepping(o, n, [0.8, 0.9], [0.001, 0.0001, 0.00005]), 100)
    path = os.path.join(HERE, "optim.npz")
    G.save(path, out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
