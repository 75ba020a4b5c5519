"""The optimiser's host side (3dal_pytorch_amd/solver.py) against the reference's record (tests/golden/optim.npz): the
schedules bit for bit, the parameter order and the BatchNorm split, the chunk table, torch.optim.Adam's checkpoint format, the
refusals, the bound symbols; and tests/solver_ref.py's restatement against the record's float64 run. No GPU."""
import ctypes
import functools
import importlib
import os

import numpy as np
import pytest
import torch

import solver_ref as T
from _common import ROOT, golden

hip = importlib.import_module("3dal_pytorch_amd._hip")
solver = importlib.import_module("3dal_pytorch_amd.solver")

ENTRIES = ("dal3_optim_partials", "dal3_optim_grad_norm", "dal3_optim_step", "dal3_optim_total_norm")
ADAM = functools.partial(torch.optim.Adam, betas=T.ADAM["betas"], amsgrad=0.0)


@pytest.fixture(autouse=True)
def _grad_enabled():
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def gold():
    return golden("optim")


class Fake:
    lr = 0
    mom = 0


def _one_cycle(target, n):
    return solver.OneCycle(target, n, T.ONE_CYCLE["lr_max"], T.ONE_CYCLE["moms"], T.ONE_CYCLE["div_factor"], T.ONE_CYCLE["pct_start"])


def _wrapper(gold, config="tt", **kw):
    true_wd, bn_wd = T.CONFIGS[config]
    model = T.build_model(gold["init"], gold["names"])
    return model, solver.OptimWrapper.create(ADAM, T.LR0, solver.get_layer_groups(model), wd=T.WD, true_wd=true_wd, bn_wd=bn_wd, **kw)


@pytest.mark.parametrize("n", [7, 20, 1000])
def test_one_cycle_table_equals_the_record_bit_for_bit(gold, n):
    want = gold[f"sched/{n}"]
    assert want.dtype == np.float64 and want.shape == (n, 2)
    table = _one_cycle(Fake(), n).table()
    assert table.dtype == np.float64 and np.array_equal(table.view(np.int64), want.view(np.int64))
    # the host route leaves the same values, step by step; int(total_step * pct_start) truncates (7 * 0.4 -> 2)
    f = Fake()
    s = _one_cycle(f, n)
    assert s.lr_phases[1][0] == int(n * 0.4)
    for i in (0, 1, int(n * 0.4), n - 1):
        s.step(i)
        assert (f.lr, f.mom) == tuple(want[i])
        assert (f.lr, f.mom) == T.one_cycle(n, i)


def test_one_cycle_of_one_step_is_refused_as_in_the_reference(gold):
    assert bool(gold["sched_1_raises"]) and "sched/1" not in gold
    with pytest.raises(AssertionError):
        _one_cycle(Fake(), 1)


def test_other_schedules_equal_the_record(gold):
    exp = solver.ExponentialDecay(Fake(), 100, 3e-4, 0.1, 0.8, staircase=True).table()
    man = solver.ManualStepping(Fake(), 100, [0.8, 0.9], [0.001, 0.0001, 0.00005]).table()
    assert np.array_equal(exp.view(np.int64), gold["sched_exp"].view(np.int64))
    assert np.array_equal(man.view(np.int64), gold["sched_manual"].view(np.int64))
    with pytest.raises(TypeError):
        solver.LRSchedulerStep(Fake(), 10, [(0, "lambda p: p")], [])


def test_parameter_order_and_batchnorm_split_equal_the_record(gold):
    model, opt = _wrapper(gold)
    by_id = {id(p): n for n, p in model.named_parameters()}
    assert [by_id[id(p)] for p in opt.params] == [str(n) for n in gold["names"]]
    assert [p.numel() for p in opt.params] == list(gold["sizes"])
    assert len(opt._groups[1]) == int(gold["n_bn"]) == 4
    bn = {id(p) for m in model.modules() if isinstance(m, solver.bn_types) for p in m.parameters()}
    assert all((id(p) in bn) == (i >= len(opt._groups[0])) for i, p in enumerate(opt.params))
    assert "frozen.weight" not in [by_id[id(p)] for p in opt.params]
    assert {1, 3, 4095, 4096, 4097, 2 * 4096 + 5} <= set(int(s) for s in gold["sizes"])
    groups = solver.split_bn_bias(solver.get_layer_groups(model))
    assert len(groups) == 2 and all(isinstance(c, solver.bn_types) for c in groups[1].children())


@pytest.mark.parametrize("config", list(T.CONFIGS))
def test_chunk_table_and_views(gold, config):
    model, opt = _wrapper(gold, config)
    rows = opt.chunk_rows()
    assert opt.n_flat % 4 == 0 and opt.n_flat == sum((int(s) + 3) // 4 * 4 for s in gold["sizes"])
    want = []
    for i, (p, off) in enumerate(zip(opt.params, opt._offsets)):
        assert off % 4 == 0 and p.grad.data_ptr() == opt._grad.data_ptr() + 4 * off and p.grad.shape == p.shape
        assert opt.state[p]["exp_avg"].data_ptr() == opt._exp_avg.data_ptr() + 4 * off
        assert opt.state[p]["exp_avg_sq"].data_ptr() == opt._exp_avg_sq.data_ptr() + 4 * off
        decay = 1 if i < len(opt._groups[0]) or T.CONFIGS[config][1] else 0
        for i0 in range(0, p.numel(), hip.OPTIM_CHUNK):
            want.append((p.data_ptr() + 4 * i0, off + i0, min(hip.OPTIM_CHUNK, p.numel() - i0), decay))
    assert rows == want
    assert [r[2] for r in rows if r[2] != hip.OPTIM_CHUNK] == [3, 1, 4095, 1, 5, 3, 3, 5, 5]      # the tails, in parameter order
    frozen = model.frozen.weight
    assert frozen.grad is None and all(not (r[0] <= frozen.data_ptr() < r[0] + 4 * r[2]) for r in rows)
    # autograd accumulates into the views in place
    loss = sum((p * p).sum() for p in opt.params)
    loss.backward()
    loss = sum(p.sum() for p in opt.params)
    loss.backward()
    for p, g in zip(opt.params, opt._grad_views):
        assert p.grad is g and torch.equal(g, 2 * p.detach() + 1)
    # a gradient that was dropped or replaced comes back into its slice; the pads are never written
    opt.params[0].grad = None
    opt.params[1].grad = torch.full_like(opt.params[1], 7.0)
    opt._adopt()
    assert opt.params[0].grad is opt._grad_views[0] and not opt._grad_views[0].any()
    assert opt.params[1].grad is opt._grad_views[1] and (opt._grad_views[1] == 7).all()
    pad = np.ones(opt.n_flat, bool)
    for p, off in zip(opt.params, opt._offsets):
        pad[off:off + p.numel()] = False
    assert pad.sum() == opt.n_flat - int(gold["sizes"].sum()) == 19 and not opt._grad.numpy()[pad].any()
    opt.zero_grad(set_to_none=True)                 # the hint is ignored: the views stay
    assert not opt._grad.any() and all(p.grad is g for p, g in zip(opt.params, opt._grad_views))


def test_state_dict_has_torch_adams_structure(gold):
    model, opt = _wrapper(gold, "cp")
    ref_model = T.build_model(gold["init"], gold["names"])
    groups = [solver.trainable_params(g) for g in solver.split_bn_bias(solver.get_layer_groups(ref_model))]
    adam = torch.optim.Adam([{"params": g, "lr": T.LR0, "weight_decay": T.WD} for g in groups], betas=T.ADAM["betas"], amsgrad=False)
    mine, want = opt.state_dict(), adam.state_dict()
    assert mine["state"] == {} == want["state"] and set(mine) == set(want)
    assert len(mine["param_groups"]) == 2
    for a, b in zip(mine["param_groups"], want["param_groups"]):
        assert set(a) == set(b) and a["params"] == b["params"]
        assert {"lr", "betas", "eps", "weight_decay", "amsgrad", "params"} <= set(a)
        assert (a["lr"], tuple(a["betas"]), a["eps"], a["weight_decay"], bool(a["amsgrad"])) == (b["lr"], tuple(b["betas"]), b["eps"], b["weight_decay"], False)
    # a stock checkpoint after two steps loads, and comes out again in the same shape
    for _ in range(2):
        for g in groups:
            for p in g:
                p.grad = torch.ones_like(p)
        adam.step()
    want = adam.state_dict()
    opt.load_state_dict(want)
    mine = opt.state_dict()
    assert opt.step_count == 2 and set(mine["state"]) == set(want["state"]) == set(range(len(opt.params)))
    for i, s in want["state"].items():
        assert set(mine["state"][i]) == set(s)
        for k in s:
            assert mine["state"][i][k].dtype == s[k].dtype and mine["state"][i][k].shape == s[k].shape and torch.equal(mine["state"][i][k], s[k]), (i, k)
    # ... and back into stock torch
    adam2 = torch.optim.Adam([{"params": g} for g in groups])
    adam2.load_state_dict(mine)
    assert adam2.param_groups[0]["betas"] == tuple(T.ADAM["betas"]) and adam2.param_groups[0]["weight_decay"] == T.WD
    # true_wd leaves 0 in the groups, as the reference's step does
    assert [g["weight_decay"] for g in _wrapper(gold, "tt")[1].state_dict()["param_groups"]] == [0, 0]
    with pytest.raises(ValueError):
        opt.load_state_dict({"state": {}, "param_groups": [dict(want["param_groups"][0], params=[0]), want["param_groups"][1]]})


def test_properties_read_and_write_the_block(gold):
    _, opt = _wrapper(gold)
    assert (opt.lr, opt.mom, opt.beta, opt.wd) == (T.LR0, 0.9, 0.99, T.WD) and opt.step_count == 0
    s = _one_cycle(opt, T.TOTAL_STEP)
    assert (opt.lr, opt.mom) == (T.ONE_CYCLE["lr_max"] / T.ONE_CYCLE["div_factor"], T.ONE_CYCLE["moms"][0])
    for t in range(T.STEPS):
        s.step(t)
        assert (opt.lr, opt.mom) == (gold["tt/lr"][t], gold["tt/mom"][t])
    opt.wd, opt.beta = 0.5, 0.75
    assert (opt.wd, opt.beta) == (0.5, 0.75)
    s.attach()
    blk = opt._blk.numpy()
    opt._flush()
    assert blk[hip.OPTIM_TOTAL_STEP] == T.TOTAL_STEP and blk[hip.OPTIM_TABLE] == opt._table.data_ptr()
    assert np.array_equal(opt._table.numpy().view(np.int64), gold["sched/20"].view(np.int64))
    assert blk[hip.OPTIM_FLAGS] == hip.OPTIM_TRUE_WD
    built = solver.build_one_cycle_optimizer(T.build_model(), dict(fixed_wd=True, amsgrad=0.0, wd=0.01))
    assert built.true_wd and built.bn_wd and (built.lr, built.mom, built.beta, built.wd) == (3e-3, 0.9, 0.99, 0.01)


def test_refusals(gold):
    model = T.build_model()
    lg = solver.get_layer_groups(model)
    with pytest.raises(ValueError, match="Adam"):
        solver.OptimWrapper.create(functools.partial(torch.optim.SGD, momentum=0.9), 1e-3, lg, wd=0.0)
    with pytest.raises(ValueError, match="Adam"):
        solver.OptimWrapper.create(torch.optim.AdamW, 1e-3, lg, wd=0.0)
    with pytest.raises(ValueError, match="amsgrad"):
        solver.OptimWrapper.create(functools.partial(torch.optim.Adam, amsgrad=1.0), 1e-3, lg, wd=0.0)
    with pytest.raises(ValueError, match="layer group"):
        solver.OptimWrapper.create(ADAM, 1e-3, lg + lg, wd=0.0)
    with pytest.raises(ValueError, match="layer group"):
        solver.OptimWrapper.create(ADAM, [1e-3, 1e-4], lg, wd=0.0)
    with pytest.raises(TypeError, match="float32"):
        solver.OptimWrapper.create(ADAM, 1e-3, solver.get_layer_groups(T.build_model().double()), wd=0.0)
    with pytest.raises(TypeError, match="float32"):
        solver.OptimWrapper.create(ADAM, 1e-3, solver.get_layer_groups(T.build_model().half()), wd=0.0)
    with pytest.raises(ValueError, match="2-norm"):
        solver.OptimWrapper.create(ADAM, 1e-3, lg, wd=0.0).clip_grad_norm(35, norm_type=1)
    with pytest.raises(RuntimeError, match="GPU"):         # no CPU fallback for the step
        solver.OptimWrapper.create(ADAM, 1e-3, solver.get_layer_groups(T.build_model()), wd=0.0).step()


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dal3.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRIES:
        assert name + "(" in header and name in hip.SIGNATURES and hasattr(lib, name), name
    assert f"#define DAL3_OPTIM_CHUNK {hip.OPTIM_CHUNK}" in header and f"#define DAL3_OPTIM_NORM_SPAN {hip.OPTIM_NORM_SPAN}" in header
    assert f"DAL3_OPTIM_TRUE_WD = {hip.OPTIM_TRUE_WD}, DAL3_OPTIM_CLIP = {hip.OPTIM_CLIP}, DAL3_OPTIM_FUSED_ZERO = {hip.OPTIM_FUSED_ZERO}" in header
    assert "dal3_optim.hip" in open(os.path.join(ROOT, "3dal_pytorch_amd", "csrc", "Makefile")).read()
    assert "} dal3_optim_chunk;" in header and hip.OptimChunk.__doc__.startswith("dal3_optim_chunk")
    fields = header[header.index("typedef struct dal3_optim_hyper"):header.index("} dal3_optim_hyper;")]
    order = ["step;", "lr, beta1, beta2, eps, wd, max_norm;", "flags;", "total_step;", "table;"]
    assert [fields.index(o) for o in order] == sorted(fields.index(o) for o in order) and hip.OPTIM_SLOTS == 10
    assert (hip.OPTIM_STEP, hip.OPTIM_LR, hip.OPTIM_MAX_NORM, hip.OPTIM_FLAGS, hip.OPTIM_TOTAL_STEP, hip.OPTIM_TABLE) == (0, 1, 6, 7, 8, 9)
    assert lib.dal3_optim_partials is not None
    fn = hip.lib().dal3_optim_partials
    assert [fn(n) for n in (0, 3, 4, 16384, 16388, -4)] == [0, 0, 1, 1, 2, 0]
    # argument checks come before any launch
    assert hip.lib().dal3_optim_grad_norm(None, 4, None, None, None) == hip.EINVAL
    assert hip.lib().dal3_optim_step(None, 1, None, None, None, 6, None, None, None) == hip.EINVAL
    assert hip.lib().dal3_optim_total_norm(None, 0, None, None) == hip.EINVAL


@pytest.mark.parametrize("config", list(T.CONFIGS))
def test_restatement_in_float64_reproduces_the_record(gold, config):
    sizes, n_bn = gold["sizes"], int(gold["n_bn"])
    r = T.run(config, gold["init"], sizes, n_bn, lambda t: T.grads_of(gold, t), torch.float64)
    clipped = 0
    for t in range(T.STEPS):
        assert r[t]["lr"] == gold[f"{config}/lr"][t] and r[t]["mom"] == gold[f"{config}/mom"][t]
        assert abs(r[t]["norm"] - gold[f"{config}/norm64"][t]) <= 1e-12 * r[t]["norm"]
        clipped += r[t]["norm"] > T.MAX_NORM
        for j, k in enumerate("pmv"):
            s = T.sums(r[t][k], sizes)
            np.testing.assert_allclose(s[:, 0], gold[f"{config}/sum64"][t, :, j], rtol=1e-11, atol=1e-18)
            np.testing.assert_allclose(s[:, 1], gold[f"{config}/sumsq64"][t, :, j], rtol=1e-11, atol=1e-300)
    assert clipped * 3 == T.STEPS
    bn0 = T.offsets(sizes)[len(sizes) - n_bn]
    for k in "pmv":
        if f"{config}/{k}32" in gold:
            truth = gold[f"{config}/{k}32"].astype(np.float64) + gold[f"{config}/{k}_d"]
            mine = r[-1][k][bn0:] if config == "tf" else r[-1][k]
            # the record keeps the truth as float32 + a float32 difference: 2^-24 of the difference
            np.testing.assert_allclose(mine, truth, rtol=0, atol=1e-7 * np.abs(gold[f"{config}/{k}_d"]).max() + 1e-300)
    # and in float32 it is as far from the truth as the reference's own float32 run, give or take
    f = T.run(config, gold["init"], sizes, n_bn, lambda t: T.grads_of(gold, t), torch.float32)
    if config == "tt":
        for k in "pmv":
            truth = gold[f"tt/{k}32"].astype(np.float64) + gold[f"tt/{k}_d"]
            ratio, m, y = T.ratios(f[-1][k], gold[f"tt/{k}32"], truth, sizes)
            assert all(ratio[q] <= 2.0 for q in T.MEASURES), (k, ratio)
