"""The detector's optimiser step on the device (det3d/solver/fastai_optim.py, learning_schedules_fastai.py,
OptimizerHook.after_train_iter, build_one_cycle_optimizer): Adam with "true" or coupled weight decay, BatchNorm parameters
in a group of their own, clip_grad_norm_ and the one-cycle schedule, with the reference's names and call shapes.

A step is two launches for any number of parameters (dal3_optim_grad_norm, dal3_optim_step of include/dal3.h), reads
nothing back and can be captured in a hipGraph: the step counter, the hyperparameters, the clip coefficient and (after
`attach()`) the whole schedule live on the device.

Storage. The optimiser owns three flat float32 buffers, gradients, exp_avg and exp_avg_sq; `p.grad`, `state[p]["exp_avg"]`
and `state[p]["exp_avg_sq"]` are views into them, so every pointer is fixed for the optimiser's life and autograd
accumulates into the existing `.grad` in place. The parameters stay where the model put them.

Differences from torch.optim.Adam, all of one origin: every parameter of the optimiser owns a gradient slice (zero when
unused) and the step count is global, not per parameter. A parameter that never receives a gradient gets the same result
as in torch (only the decay applies); one that receives its first gradient late has its bias corrections at the global
step. The gradient norm is summed in float64, so gradients whose squares overflow float32 still have a finite norm.

Not built: FastAIMixedOptim (fp16 master copies), moving_average, amsgrad, per-group learning rates, schedule phases given
as strings to eval."""
import functools

import numpy as np
import torch
from torch import nn

from . import _hip as hip

bn_types = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.modules.batchnorm._BatchNorm)


# ---------------------------------------------------------------------------------------------- layer groups
def flatten_model(m):
    """the leaf modules of `m` in definition order"""
    children = list(m.children())
    return sum(map(flatten_model, children), []) if children else [m]


def get_layer_groups(m):
    return [nn.Sequential(*flatten_model(m))]


def split_bn_bias(layer_groups):
    """per layer group: its non-BatchNorm children, then its BatchNorm children, each as one nn.Sequential"""
    split_groups = []
    for group in layer_groups:
        rest, bn = [], []
        for c in group.children():
            (bn if isinstance(c, bn_types) else rest).append(c)
        split_groups += [nn.Sequential(*rest), nn.Sequential(*bn)]
    return split_groups


def trainable_params(m):
    return [p for p in m.parameters() if p.requires_grad]


def listify(p=None, q=None):
    """`p` as a list of the length of `q` (an int or a list)"""
    if p is None:
        p = []
    elif isinstance(p, str) or not isinstance(p, (list, tuple)):
        p = [p]
    n = q if isinstance(q, int) else len(p) if q is None else len(q)
    p = list(p)
    if len(p) == 1:
        p = p * n
    assert len(p) == n, f"List len mismatch ({len(p)} vs {n})"
    return p


# ---------------------------------------------------------------------------------------------- the optimiser
_ADAM_KEYWORDS = {"lr", "betas", "eps", "weight_decay", "amsgrad", "foreach", "capturable", "fused", "maximize", "differentiable"}


def _adam_keywords(opt_func):
    """the keywords of torch.optim.Adam or of a functools.partial over it; anything else is refused"""
    func, kw = opt_func, {}
    if isinstance(opt_func, functools.partial):
        if opt_func.args:
            raise ValueError("opt_func: a partial with positional arguments is not supported")
        func, kw = opt_func.func, dict(opt_func.keywords)
    if func is not torch.optim.Adam:
        raise ValueError(f"opt_func must be torch.optim.Adam or a partial over it (the device step is Adam), got {func!r}")
    unknown = set(kw) - _ADAM_KEYWORDS
    if unknown:
        raise ValueError(f"opt_func: unknown Adam keywords {sorted(unknown)}")
    if kw.get("amsgrad"):
        raise ValueError("amsgrad is not built: the device step keeps no max_exp_avg_sq (every config of the detector has amsgrad=0.0)")
    for k in ("maximize", "differentiable"):
        if kw.get(k):
            raise ValueError(f"{k}=True is not supported by the device step")
    if kw.get("weight_decay"):
        raise ValueError("give the weight decay as OptimWrapper's wd, not as Adam's weight_decay")
    return kw


class OptimWrapper:
    """OptimWrapper of the reference over a device Adam. `fused_zero=True`: the step leaves the gradients zeroed (zero_grad
    then does nothing), which saves the memset of the flat buffer."""

    def __init__(self, groups, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0, true_wd=False, bn_wd=True, fused_zero=False,
                 opt_func=torch.optim.Adam):
        if len(groups) != 2:
            raise ValueError("more than one layer group (per-group learning rates) is not built: pass get_layer_groups(model)")
        seen, self._groups = set(), []
        for g in groups:
            ps = [p for p in g if id(p) not in seen and not seen.add(id(p))]
            self._groups.append(ps)
        self.params = self._groups[0] + self._groups[1]
        if not self.params:
            raise ValueError("the layer groups hold no trainable parameter")
        dev = self.params[0].device
        for p in self.params:
            if p.dtype != torch.float32:
                raise TypeError(f"parameter of dtype {p.dtype}: the device step takes float32 parameters only "
                                "(FastAIMixedOptim's fp16 master copies are not built)")
            if p.device != dev:
                raise ValueError("all parameters must be on one device")
            if not p.is_contiguous():
                raise ValueError("parameters must be contiguous")
        self.device, self.true_wd, self.bn_wd, self.fused_zero, self.opt_func = dev, bool(true_wd), bool(bn_wd), bool(fused_zero), opt_func
        self.max_norm = None                # a number: every step clips to it (train_iter sets it)
        self._one_shot_clip = self._norm_done = False
        self._table = None
        # the flat buffers and the views
        self._offsets, off = [], 0
        for p in self.params:
            self._offsets.append(off)
            off += (p.numel() + 3) // 4 * 4
        self.n_flat = off
        self._grad, self._exp_avg, self._exp_avg_sq = (torch.zeros(off, dtype=torch.float32, device=dev) for _ in range(3))
        view = lambda buf, p, o: buf[o:o + p.numel()].view(p.shape)
        self._grad_views = [view(self._grad, p, o) for p, o in zip(self.params, self._offsets)]
        self.state = {p: {"exp_avg": view(self._exp_avg, p, o), "exp_avg_sq": view(self._exp_avg_sq, p, o)}
                      for p, o in zip(self.params, self._offsets)}
        for p, g in zip(self.params, self._grad_views):
            if p.grad is not None:
                g.copy_(p.grad)
            p.grad = g
        self._n_partials = -(-off // hip.OPTIM_NORM_SPAN)
        self._partials = torch.zeros(self._n_partials, dtype=torch.float64, device=dev)
        self._norm = torch.zeros((), dtype=torch.float32, device=dev)
        # the hyperparameter block: slot 0 (the step counter) belongs to the device, the others to the host mirror
        self._blk = torch.zeros(hip.OPTIM_SLOTS, dtype=torch.int64, device=dev)
        self._host = np.zeros(hip.OPTIM_SLOTS, np.int64)
        self._host_f = self._host.view(np.float64)
        self._host_f[hip.OPTIM_LR:hip.OPTIM_MAX_NORM + 1] = [listify(lr, 1)[0], betas[0], betas[1], eps, wd, 0.0]
        self._dirty = set(range(1, hip.OPTIM_SLOTS))
        self._set_flags()
        self._ptrs = None
        self._build_table()

    @classmethod
    def create(cls, opt_func, lr, layer_groups, wd=0.0, true_wd=False, bn_wd=True, fused_zero=False):
        """OptimWrapper.create of the reference: `opt_func` is torch.optim.Adam or the reference's
        partial(torch.optim.Adam, betas=..., amsgrad=...), whose keywords are read."""
        kw = _adam_keywords(opt_func)
        if len(layer_groups) != 1 or (isinstance(lr, (list, tuple)) and len(lr) != 1):
            raise ValueError("more than one layer group (per-group learning rates) is not built: pass get_layer_groups(model)")
        groups = [trainable_params(g) for g in split_bn_bias(layer_groups)]
        return cls(groups, lr, betas=kw.get("betas", (0.9, 0.999)), eps=kw.get("eps", 1e-8), wd=wd, true_wd=true_wd, bn_wd=bn_wd,
                   fused_zero=fused_zero, opt_func=opt_func)

    def __repr__(self):
        return (f"OptimWrapper over a device Adam of {len(self.params)} parameters ({self.n_flat} flat elements).\n"
                f"True weight decay: {self.true_wd}")

    # ---- the device block
    def _set_flags(self):
        clip = self.max_norm is not None or self._one_shot_clip
        flags = (hip.OPTIM_TRUE_WD if self.true_wd else 0) | (hip.OPTIM_CLIP if clip else 0) | (hip.OPTIM_FUSED_ZERO if self.fused_zero else 0)
        if self._host[hip.OPTIM_FLAGS] != flags:
            self._host[hip.OPTIM_FLAGS] = flags
            self._dirty.add(hip.OPTIM_FLAGS)

    def _flush(self):
        """the host's changed slots to the device: one scalar fill each, stream-ordered, nothing read back (a copy from
        pageable host memory would wait for the stream)"""
        for slot in sorted(self._dirty):
            if hip.OPTIM_LR <= slot <= hip.OPTIM_MAX_NORM:
                self._blk.view(torch.float64)[slot].fill_(float(self._host_f[slot]))
            else:
                self._blk[slot].fill_(int(self._host[slot]))
        self._dirty.clear()

    def _get(self, slot):
        self._flush()
        return float(self._blk.view(torch.float64)[slot])

    def _set(self, slot, val):
        val = float(val)
        if self._host_f[slot] != val:
            self._host_f[slot] = val
            self._dirty.add(slot)

    @property
    def lr(self):
        """the learning rate in the device block: the last one a step took when a schedule table is attached"""
        return self._get(hip.OPTIM_LR)

    @lr.setter
    def lr(self, val):
        self._set(hip.OPTIM_LR, listify(val, 1)[0])

    @property
    def mom(self):
        return self._get(hip.OPTIM_BETA1)

    @mom.setter
    def mom(self, val):
        self._set(hip.OPTIM_BETA1, listify(val, 1)[0])

    @property
    def beta(self):
        return self._get(hip.OPTIM_BETA2)

    @beta.setter
    def beta(self, val):
        if val is not None:
            self._set(hip.OPTIM_BETA2, listify(val, 1)[0])

    @property
    def wd(self):
        return self._get(hip.OPTIM_WD)

    @wd.setter
    def wd(self, val):
        self._set(hip.OPTIM_WD, listify(val, 1)[0])

    @property
    def step_count(self):
        """steps taken so far (reads the device counter: synchronises)"""
        return int(self._blk[hip.OPTIM_STEP])

    def attach_table(self, table):
        """(total_step, 2) float64 rows of (lr, beta1) for step 1, 2, ...: the device counter picks the row from now on
        (the last row once it is past the end). None detaches it."""
        if table is None:
            self._table = None
            self._host[hip.OPTIM_TOTAL_STEP] = self._host[hip.OPTIM_TABLE] = 0
        else:
            t = np.ascontiguousarray(np.asarray(table, np.float64))
            if t.ndim != 2 or t.shape[1] != 2 or t.shape[0] < 1:
                raise ValueError("the schedule table must be (total_step, 2) rows of (lr, mom)")
            self._table = torch.from_numpy(t).to(self.device)
            self._host[hip.OPTIM_TOTAL_STEP], self._host[hip.OPTIM_TABLE] = t.shape[0], self._table.data_ptr()
        self._dirty.update((hip.OPTIM_TOTAL_STEP, hip.OPTIM_TABLE))

    # ---- the chunk table
    def _decay_flag(self, group):
        return 1 if group == 0 or self.bn_wd else 0

    def _build_table(self):
        rows = []
        for i, (p, off) in enumerate(zip(self.params, self._offsets)):
            decay = self._decay_flag(0 if i < len(self._groups[0]) else 1)
            base, n = p.data_ptr(), p.numel()
            for i0 in range(0, n, hip.OPTIM_CHUNK):
                rows.append((base + 4 * i0, off + i0, min(hip.OPTIM_CHUNK, n - i0), decay))
        arr = (hip.OptimChunk * len(rows))(*rows)
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self._chunks = host.to(self.device)
        self._n_chunks = len(rows)
        self._ptrs = [p.data_ptr() for p in self.params]

    def chunk_rows(self):
        """the chunk table as the host built it: (parameter pointer, flat offset, count, decay flag) per row"""
        raw = self._chunks.cpu().numpy().tobytes()
        arr = (hip.OptimChunk * self._n_chunks).from_buffer_copy(raw)
        return [(r.param, r.offset, r.count, r.decay) for r in arr]

    def _adopt(self):
        """Before a launch: every `.grad` must still be the optimiser's view and every parameter where the table says. A
        gradient that something replaced (zero_grad(set_to_none=True) on the model, an assignment) is copied into its
        slice and the view put back; parameters that moved (`model.to`, `p.data = ...`) get a new table."""
        moved = False
        for p, g, ptr in zip(self.params, self._grad_views, self._ptrs):
            if p.grad is not g:
                if p.grad is None:
                    g.zero_()
                else:
                    g.copy_(p.grad)
                p.grad = g
            if p.data_ptr() != ptr:
                moved = True
        if moved:
            self._build_table()

    # ---- torch.optim's methods
    def zero_grad(self, set_to_none=False):
        """one memset of the flat gradient buffer; nothing under fused_zero (the step has left it zeroed). `set_to_none` is
        accepted and ignored: the gradients are the views the device step reads, they are zeroed in place."""
        if not self.fused_zero:
            self._grad.zero_()

    def _launch_norm(self):
        hip.require_gpu(self._grad, "the optimiser's state")
        self._adopt()
        self._flush()
        hip.check(hip.lib().dal3_optim_grad_norm(hip.ptr(self._grad), self.n_flat, hip.ptr(self._blk), hip.ptr(self._partials), hip.stream()))
        self._norm_done = True

    def clip_grad_norm(self, max_norm, norm_type=2):
        """clip_grad_norm_ of the iteration's gradients, fused into the next step(): the norm is taken now and returned as a
        device scalar (one more small launch), the scaling happens in the step's kernel."""
        if float(norm_type) != 2.0:
            raise ValueError("only the 2-norm is built")
        self._set(hip.OPTIM_MAX_NORM, max_norm)
        self._one_shot_clip = True
        self._set_flags()
        if not self._norm_done:
            self._launch_norm()
        hip.check(hip.lib().dal3_optim_total_norm(hip.ptr(self._partials), self._n_partials, hip.ptr(self._norm), hip.stream()))
        return self._norm

    def total_norm(self):
        """the 2-norm of the gradients the last step (or clip_grad_norm) saw, as a device scalar"""
        hip.check(hip.lib().dal3_optim_total_norm(hip.ptr(self._partials), self._n_partials, hip.ptr(self._norm), hip.stream()))
        return self._norm

    def step(self):
        """decay, clip (when armed) and Adam for every parameter: two launches, or one after clip_grad_norm()"""
        if self.max_norm is not None:
            self._set(hip.OPTIM_MAX_NORM, self.max_norm)
        self._set_flags()
        if not self._norm_done:
            self._launch_norm()
        else:
            self._flush()
        hip.check(hip.lib().dal3_optim_step(hip.ptr(self._chunks), self._n_chunks, hip.ptr(self._grad), hip.ptr(self._exp_avg),
                                            hip.ptr(self._exp_avg_sq), self.n_flat, hip.ptr(self._partials), hip.ptr(self._blk),
                                            hip.stream()))
        self._norm_done = False
        if self._one_shot_clip:
            self._one_shot_clip = False
            self._set_flags()

    def clear(self):
        """reset the moments and the step counter"""
        self._exp_avg.zero_()
        self._exp_avg_sq.zero_()
        self._blk[hip.OPTIM_STEP] = 0

    # ---- checkpoints, in torch.optim.Adam's own format
    def _group_dicts(self):
        self._flush()
        h = self._blk.cpu().numpy().view(np.float64)
        template = torch.optim.Adam([torch.zeros(1)]).param_groups[0]
        out, first = [], 0
        for gi, ps in enumerate(self._groups):
            g = {k: v for k, v in template.items() if k != "params"}
            decays = (not self.true_wd) and self._decay_flag(gi)
            g.update(lr=float(h[hip.OPTIM_LR]), betas=(float(h[hip.OPTIM_BETA1]), float(h[hip.OPTIM_BETA2])), eps=float(h[hip.OPTIM_EPS]),
                     weight_decay=float(h[hip.OPTIM_WD]) if decays else 0, amsgrad=False)
            g["params"] = list(range(first, first + len(ps)))
            first += len(ps)
            out.append(g)
        return out

    @property
    def param_groups(self):
        groups = self._group_dicts()
        for g, ps in zip(groups, self._groups):
            g["params"] = ps
        return groups

    def state_dict(self):
        """torch.optim.Adam's format: before the first step no parameter has state, after it every parameter has (every one
        owns a gradient slice), all with the global step."""
        step = self.step_count
        state = {}
        if step > 0:
            for i, p in enumerate(self.params):
                s = self.state[p]
                state[i] = {"step": torch.tensor(float(step)), "exp_avg": s["exp_avg"].detach().clone(),
                            "exp_avg_sq": s["exp_avg_sq"].detach().clone()}
        return {"state": state, "param_groups": self._group_dicts()}

    def load_state_dict(self, sd):
        """A checkpoint of this class or of torch.optim.Adam over the same parameter order (the reference's
        save_checkpoint). The moments and the step come from it (the largest step, where torch kept one per parameter;
        parameters without state start from zero moments), lr / betas / eps from its first group; the weight decay stays
        this wrapper's, as in the reference, whose true_wd step leaves 0 in the groups."""
        groups = sd["param_groups"]
        if [len(g["params"]) for g in groups] != [len(ps) for ps in self._groups]:
            raise ValueError(f"the checkpoint's groups hold {[len(g['params']) for g in groups]} parameters, this optimiser's "
                             f"{[len(ps) for ps in self._groups]}")
        if any(g.get("amsgrad") for g in groups):
            raise ValueError("the checkpoint was written with amsgrad, which is not built")
        ids = [i for g in groups for i in g["params"]]
        self._exp_avg.zero_()
        self._exp_avg_sq.zero_()
        step = 0
        for p, i in zip(self.params, ids):
            s = sd["state"].get(i)
            if not s:
                continue
            if s["exp_avg"].shape != p.shape:
                raise ValueError(f"parameter {i}: the checkpoint's exp_avg is {tuple(s['exp_avg'].shape)}, the parameter {tuple(p.shape)}")
            self.state[p]["exp_avg"].copy_(s["exp_avg"])
            self.state[p]["exp_avg_sq"].copy_(s["exp_avg_sq"])
            step = max(step, int(float(s["step"])))
        self._blk[hip.OPTIM_STEP] = step
        g0 = groups[0]
        self.lr, self.mom, self.beta = g0["lr"], g0["betas"][0], g0["betas"][1]
        self._set(hip.OPTIM_EPS, g0["eps"])
        self._norm_done = False


def build_one_cycle_optimizer(model, optimizer_config):
    """the reference's builder: `optimizer_config` has fixed_wd, amsgrad and wd (attributes or keys)"""
    get = (lambda k: optimizer_config[k]) if isinstance(optimizer_config, dict) else (lambda k: getattr(optimizer_config, k))
    if get("fixed_wd"):
        opt_func = functools.partial(torch.optim.Adam, betas=(0.9, 0.99), amsgrad=get("amsgrad"))
    else:
        opt_func = functools.partial(torch.optim.Adam, amsgrad=get("amsgrad"))
    return OptimWrapper.create(opt_func, 3e-3, get_layer_groups(model), wd=get("wd"), true_wd=get("fixed_wd"), bn_wd=True)


def train_iter(optimizer, loss, grad_clip=None):
    """OptimizerHook.after_train_iter: zero_grad -> backward -> clip -> step. `grad_clip` is the config's
    dict(max_norm=35, norm_type=2); the clip is fused into the step, which stays two launches."""
    optimizer.zero_grad()
    loss.backward()
    if grad_clip is not None:
        if float(grad_clip.get("norm_type", 2)) != 2.0:
            raise ValueError("only the 2-norm is built")
        optimizer.max_norm = float(grad_clip["max_norm"])
    else:
        optimizer.max_norm = None
    optimizer.step()


# ---------------------------------------------------------------------------------------------- schedules
def annealing_cos(start, end, pct):
    """cosine from `start` to `end` as pct goes from 0 to 1"""
    cos_out = np.cos(np.pi * pct) + 1
    return end + (start - end) / 2 * cos_out


class _Recorder:
    """stands in for the optimiser while a schedule is evaluated"""

    def __init__(self, lr, mom):
        self.lr, self.mom = lr, mom


class LRSchedulerStep:
    """Phases of (start fraction, function of the phase's progress in [0, 1)) for lr and for mom. step(global_step) is the
    host route (it sets the optimiser's lr / mom); attach() evaluates every step once and hands the table to the device,
    whose own counter then drives the schedule."""

    def __init__(self, fai_optimizer, total_step, lr_phases, mom_phases):
        self.optimizer, self.total_step = fai_optimizer, total_step
        self.lr_phases, self.mom_phases = self._phases(lr_phases, total_step), self._phases(mom_phases, total_step)
        assert self.lr_phases[0][0] == 0
        if self.mom_phases:
            assert self.mom_phases[0][0] == 0

    @staticmethod
    def _phases(phases, total_step):
        phases, out = list(phases), []
        for i, (start, func) in enumerate(phases):
            if not callable(func):
                raise TypeError("a schedule phase must be a callable (strings to eval are not supported)")
            first = int(start * total_step)
            if out:
                assert out[-1][0] < first
            last = int(phases[i + 1][0] * total_step) if i < len(phases) - 1 else total_step
            out.append((first, last, func))
        return out

    def _apply(self, target, step):
        lr = mom = None
        for start, end, func in self.lr_phases:
            if step >= start:
                lr = func((step - start) / (end - start))
        if lr is not None:
            target.lr = lr
        for start, end, func in self.mom_phases:
            if step >= start:
                mom = func((step - start) / (end - start))
        if mom is not None:
            target.mom = mom

    def step(self, step):
        self._apply(self.optimizer, step)

    def table(self, lr=None, mom=None):
        """(total_step, 2) float64: what step(0), step(1), ... leave in (lr, mom), starting from the given values (a phase
        that does not cover a step leaves the value before it)"""
        rec = _Recorder(self.optimizer.lr if lr is None else lr, self.optimizer.mom if mom is None else mom)
        out = np.zeros((self.total_step, 2), np.float64)
        for s in range(self.total_step):
            self._apply(rec, s)
            out[s] = rec.lr, rec.mom
        return out

    def attach(self):
        self.optimizer.attach_table(self.table())
        return self


class OneCycle(LRSchedulerStep):
    def __init__(self, fai_optimizer, total_step, lr_max, moms, div_factor, pct_start):
        self.lr_max, self.moms, self.div_factor, self.pct_start = lr_max, moms, div_factor, pct_start
        low_lr = lr_max / div_factor
        lr_phases = ((0, functools.partial(annealing_cos, low_lr, lr_max)),
                     (pct_start, functools.partial(annealing_cos, lr_max, low_lr / 1e4)))
        mom_phases = ((0, functools.partial(annealing_cos, *moms)), (pct_start, functools.partial(annealing_cos, *moms[::-1])))
        fai_optimizer.lr, fai_optimizer.mom = low_lr, moms[0]
        super().__init__(fai_optimizer, total_step, lr_phases, mom_phases)


class ExponentialDecay(LRSchedulerStep):
    def __init__(self, fai_optimizer, total_step, initial_learning_rate, decay_length, decay_factor, staircase=True):
        assert 0 < decay_length < 1
        lr_phases = []
        if staircase:
            assert int(decay_length * total_step) > 0
            step, stage = 0, 1
            while step <= total_step:
                lr_phases.append((step / total_step, lambda p, _d=initial_learning_rate * stage: _d))
                stage *= decay_factor
                step += int(decay_length * total_step)
        else:
            lr_phases.append((0, lambda p: pow(decay_factor, p / decay_length)))
        super().__init__(fai_optimizer, total_step, lr_phases, [])


class ManualStepping(LRSchedulerStep):
    def __init__(self, fai_optimizer, total_step, boundaries, rates):
        assert all(0 < b < 1 for b in boundaries)
        assert len(boundaries) + 1 == len(rates)
        lr_phases = [(start, lambda p, _d=rate: _d) for start, rate in zip([0.0] + list(boundaries), rates)]
        super().__init__(fai_optimizer, total_step, lr_phases, [])
