"""What the solver tests share: the small seeded model of tests/golden/optim.npz, the record's layout, a stock-torch
restatement of the reference's iteration (OneCycle.step -> clip_grad_norm_ -> OptimWrapper.step over torch.optim.Adam's
arithmetic) that runs in float32 or float64, and the measures and the bar of the GPU tests.

The record (tests/golden/gen_optim.py writes it from the reference's own two solver files). Parameter order `names`, the
tensors' `sizes`, `n_bn` BatchNorm tensors at the end; `init` the float32 parameters, flat in that order (as every flat
array here: the tensors back to back, unpadded); the float32 gradients of step t are grad_q[t] * grad_scale[t] (int8 times a
power of two: exact); per configuration c of CONFIGS and per step norm32 / norm64 (clip_grad_norm_'s return in the float32
and the .double() run), lr, mom, and sum64 / sumsq64 (steps, tensors, 3): the float64 run's sum and sum of squares of every
parameter, exp_avg and exp_avg_sq tensor; after the last step the float32 run's flat p32 / m32 / v32 with the float64 run as
a float32 difference p_d / m_d / v_d (truth = x32 + x_d). A committed file may not exceed 1 MiB, so the full arrays are kept
where they carry something new: all three for `tt`; for `tf`, which differs from `tt` in nothing but the BatchNorm
parameters, those (p32 / p_d are the last n_bn tensors' elements); the parameters for `cp`. Every other step and array of the
float64 run is held by its sums, which this file's restatement reproduces (tests/test_solver_cpu.py)."""
import numpy as np
import torch
from torch import nn

STEPS, TOTAL_STEP, MAX_NORM = 12, 20, 35.0
ONE_CYCLE = dict(lr_max=0.003, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4)
ADAM = dict(betas=(0.9, 0.99), eps=1e-8)
LR0, WD = 3e-3, 0.01
# name -> (true_wd, bn_wd)
CONFIGS = {"tt": (True, True), "tf": (True, False), "cp": (False, True)}
SCHEDULE_STEPS = (1, 7, 20, 1000)

# The GPU tests' bar, by the rule written beside pillars_ref.BARS: each measure of the kernel's error against the float64
# record is held to BAR x the same measure of the reference's own float32 run. BAR = 2 x the worst ratio measured on the
# MI355X (profiles/optim_measured.json, DAL3_OPTIM_RECORD over tests/test_gpu_solver.py, 16 rows), rounded up to one
# decimal; it may never exceed 4.3, the loosest bar a kernel here carries. The margin covers the different summation order
# of the norm and fused multiply-adds on either side. Recorded at worst: 1.002 (tt/p, rms; the max measures are 1.000 or
# below in every row: the norm is the float64 sum rounded once, and the element arithmetic is torch's, operation by
# operation) -> 2 x 1.002 = 2.004 -> 2.1.
BAR = 2.1
MEASURES = ("max", "rms")
FLOOR = 1e-30


class Net(nn.Module):
    """never run forward: its parameters only. Tensor sizes 3, 1, 3, 3, 4095, 4096, 5, 5, 4097, 2 * 4096 + 5 and a frozen
    7; BatchNorm leaves at two depths."""

    def __init__(self):
        super().__init__()
        self.fc0 = nn.Linear(3, 1)
        self.bn0 = nn.BatchNorm1d(3)
        self.fc1 = nn.Linear(4095, 1, bias=False)
        self.block = nn.Sequential(nn.Linear(64, 64, bias=False), nn.BatchNorm1d(5))
        self.frozen = nn.Linear(7, 1, bias=False)
        self.frozen.weight.requires_grad_(False)
        self.fc3 = nn.Linear(4097, 1, bias=False)
        self.fc4 = nn.Linear(8197, 1, bias=False)


def build_model(init=None, names=None):
    """the model, with the record's parameters when given (flat `init` in the order `names`)"""
    torch.manual_seed(0)
    m = Net()
    if init is not None:
        named = dict(m.named_parameters())
        off = 0
        with torch.no_grad():
            for n in names:
                p = named[str(n)]
                p.copy_(torch.from_numpy(np.asarray(init[off:off + p.numel()])).view(p.shape))
                off += p.numel()
        assert off == len(init)
    return m


def seeded_init(model):
    """float32 values for every trainable parameter: N(0, 0.1), BatchNorm weights around 1"""
    rng = np.random.RandomState(0)
    with torch.no_grad():
        for n, p in model.named_parameters():
            v = (0.1 * rng.standard_normal(p.numel())).astype(np.float32)
            if isinstance(dict(model.named_modules())[n.rsplit(".", 1)[0]], nn.modules.batchnorm._BatchNorm) and n.endswith("weight"):
                v += 1
            p.copy_(torch.from_numpy(v).view(p.shape))


def seeded_grads(n):
    """-> grad_q (STEPS, n) int8, grad_scale (STEPS) float32. The norms are about 16 (no clip at 35) and, every third step,
    32 times that (about 520: clipped)."""
    rng = np.random.RandomState(1)
    q = np.clip(np.rint(29.0 * rng.standard_normal((STEPS, n))), -127, 127).astype(np.int8)
    scale = np.array([2.0 ** -8 * (32.0 if t % 3 == 1 else 1.0) for t in range(STEPS)], np.float32)
    return q, scale


def grads_of(g, t):
    return g["grad_q"][t].astype(np.float32) * g["grad_scale"][t]


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))])


def flat(tensors):
    return np.concatenate([np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t).reshape(-1) for t in tensors])


def run(config, init, sizes, n_bn, grad_fn, dtype, steps=STEPS, max_norm=MAX_NORM):
    """the reference's iteration restated in stock torch ops, in `dtype`. init: flat parameters; grad_fn(t) -> the flat
    float32 gradients of step t; max_norm None: no clip. -> per step {norm, lr, mom, p, m, v, g} (flat numpy; g the gradients after the clip)"""
    true_wd, bn_wd = CONFIGS[config]
    off = offsets(sizes)
    T = len(sizes)
    ps = [torch.tensor(np.asarray(init[off[i]:off[i + 1]]), dtype=dtype) for i in range(T)]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    decays = [i < T - n_bn or bn_wd for i in range(T)]
    beta2, eps = ADAM["betas"][1], ADAM["eps"]
    out = []
    for t in range(steps):
        lr, mom = one_cycle(TOTAL_STEP, t)
        g_flat = grad_fn(t)
        gs = [torch.tensor(g_flat[off[i]:off[i + 1]], dtype=dtype) for i in range(T)]
        # clip_grad_norm_(max_norm=35, norm_type=2)
        norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g, 2.0) for g in gs]), 2.0)
        if max_norm is not None:
            coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
            for g in gs:
                g.mul_(coef)
        # OptimWrapper.step
        for i in range(T):
            if true_wd and decays[i]:
                ps[i].mul_(1 - WD * lr)
        step = t + 1
        bc1, bc2 = 1 - mom ** step, 1 - beta2 ** step
        for i in range(T):
            g = gs[i]
            if not true_wd and decays[i]:
                g = g.add(ps[i], alpha=WD)
            ms[i].lerp_(g, 1 - mom)
            vs[i].mul_(beta2).addcmul_(g, g, value=1 - beta2)
            denom = (vs[i].sqrt() / (bc2 ** 0.5)).add_(eps)
            ps[i].addcdiv_(ms[i], denom, value=-(lr / bc1))
        out.append(dict(norm=float(norm), lr=lr, mom=mom, p=flat(ps), m=flat(ms), v=flat(vs), g=flat(gs)))
    return out


def annealing_cos(start, end, pct):
    return end + (start - end) / 2 * (np.cos(np.pi * pct) + 1)


def one_cycle(total_step, step, lr_max=ONE_CYCLE["lr_max"], moms=ONE_CYCLE["moms"], div_factor=ONE_CYCLE["div_factor"],
              pct_start=ONE_CYCLE["pct_start"]):
    """(lr, mom) that OneCycle leaves after step(`step`)"""
    a1 = int(total_step * pct_start)
    low = lr_max / div_factor
    if step >= a1:
        pct = (step - a1) / (total_step - a1)
        return float(annealing_cos(lr_max, low / 1e4, pct)), float(annealing_cos(moms[1], moms[0], pct))
    pct = step / a1
    return float(annealing_cos(low, lr_max, pct)), float(annealing_cos(moms[0], moms[1], pct))


def sums(x, sizes):
    """(tensors, 2) float64: sum and sum of squares per tensor of a flat array"""
    off = offsets(sizes)
    x = np.asarray(x, np.float64)
    return np.array([[x[off[i]:off[i + 1]].sum(), (x[off[i]:off[i + 1]] ** 2).sum()] for i in range(len(sizes))])


def scales(truth, sizes):
    """per element: the largest |truth| of the element's tensor"""
    off = offsets(sizes)
    s = np.empty(len(truth))
    for i in range(len(sizes)):
        s[off[i]:off[i + 1]] = np.abs(truth[off[i]:off[i + 1]]).max()
    return s


def judge(got, truth, sizes):
    """per element, each error over its tensor's largest |truth|: the largest and the root mean square"""
    truth = np.asarray(truth, np.float64)
    d = (np.asarray(got, np.float64) - truth) / np.maximum(scales(truth, sizes), FLOOR)
    return {"max": float(np.abs(d).max()), "rms": float(np.sqrt((d ** 2).mean()))}


def ratios(got, f32, truth, sizes):
    """each measure of got over the same measure of the float32 reference run -> (ratios, measured, yardstick)"""
    m, y = judge(got, truth, sizes), judge(f32, truth, sizes)
    return {k: m[k] / max(y[k], FLOOR) for k in MEASURES}, m, y
