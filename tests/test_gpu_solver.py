"""The optimiser step on the GPU (3dal_pytorch_amd/solver.py; dal3_optim_grad_norm, dal3_optim_step, dal3_optim_total_norm)
against the reference's record (tests/golden/optim.npz, laid out in tests/solver_ref.py): lr, mom and the step count exactly,
parameters, moments and the norm in multiples of the reference's own float32 error against float64 (solver_ref.BAR), chunk
seams and pads, non-finite gradients, reproducibility, the captured graph, checkpoints, the frozen parameter, and one
iteration of the small VoxelNet. DAL3_OPTIM_RECORD=<path> writes every figure held (how profiles/optim_measured.json is
made).

Measured on the MI355X (profiles/optim_measured.json): the worst ratio of the 16 rows is 1.002 (tt/p, rms), the norm's 1.000;
the bar is 2.1."""
import ctypes
import functools
import importlib
import json
import os

import numpy as np
import pytest
import torch

import solver_ref as T
from _common import golden

hip = importlib.import_module("3dal_pytorch_amd._hip")
solver = importlib.import_module("3dal_pytorch_amd.solver")
pytestmark = pytest.mark.gpu

_RECORD = {}
ADAM = functools.partial(torch.optim.Adam, betas=T.ADAM["betas"], amsgrad=0.0)
CLIP = dict(max_norm=T.MAX_NORM, norm_type=2)


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    path = os.environ.get("DAL3_OPTIM_RECORD")
    if path and _RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _grad_enabled():
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def gold():
    return golden("optim")


def _make(gold, config, init=None, **kw):
    true_wd, bn_wd = T.CONFIGS[config]
    model = T.build_model(gold["init"] if init is None else init, gold["names"]).cuda()
    opt = solver.OptimWrapper.create(ADAM, T.LR0, solver.get_layer_groups(model), wd=T.WD, true_wd=true_wd, bn_wd=bn_wd, **kw)
    sched = solver.OneCycle(opt, T.TOTAL_STEP, T.ONE_CYCLE["lr_max"], T.ONE_CYCLE["moms"], T.ONE_CYCLE["div_factor"], T.ONE_CYCLE["pct_start"])
    return model, opt, sched


def _index(opt):
    """positions of the tensors' elements in the padded flat buffers, in parameter order"""
    return np.concatenate([np.arange(o, o + p.numel()) for p, o in zip(opt.params, opt._offsets)])


def _feed(opt, g):
    buf = np.zeros(opt.n_flat, np.float32)
    buf[_index(opt)] = g
    opt._grad.copy_(torch.from_numpy(buf))


def _state(opt):
    idx = _index(opt)
    return dict(p=T.flat(opt.params), m=opt._exp_avg.cpu().numpy()[idx], v=opt._exp_avg_sq.cpu().numpy()[idx], g=opt._grad.cpu().numpy()[idx])


def _pads_are_zero(opt):
    pad = np.ones(opt.n_flat, bool)
    pad[_index(opt)] = False
    assert pad.sum() == 19
    for buf in (opt._grad, opt._exp_avg, opt._exp_avg_sq):
        a = buf.cpu().numpy()[pad]
        assert not a.any() and not np.signbit(a).any()


def _run(gold, config, route="table"):
    """12 iterations on the recorded gradients. route 'table': the schedule attached, the clip armed for good (no host
    value changes between steps); 'host': OneCycle.step(t) and clip_grad_norm() every iteration."""
    model, opt, sched = _make(gold, config)
    if route == "table":
        sched.attach()
        opt.max_norm = T.MAX_NORM
    steps = []
    for t in range(T.STEPS):
        g = T.grads_of(gold, t)
        opt.zero_grad()
        _feed(opt, g)
        if route == "host":
            sched.step(t)
            norm = float(opt.clip_grad_norm(**CLIP))
            opt.step()
            assert float(opt.total_norm()) == norm
        else:
            opt.step()
            norm = float(opt.total_norm())
        steps.append(dict(norm=norm, lr=opt.lr, mom=opt.mom, step=opt.step_count, fed=g, **_state(opt)))
        if t == 5:
            steps[-1]["sd"] = opt.state_dict()
    return model, opt, steps


@pytest.fixture(scope="module")
def runs(gold):
    return {c: _run(gold, c) for c in T.CONFIGS}


def _hold(row, got, f32, truth, sizes):
    ratio, m, y = T.ratios(got, f32, truth, sizes)
    _RECORD[row] = {"measured": m, "yardstick": y, "ratio": ratio}
    for k in T.MEASURES:
        print(f"{row:32s} {k:4s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:7.3f}  bar {T.BAR:g}")
    bad = [(k, m[k], ratio[k]) for k in T.MEASURES if not ratio[k] <= T.BAR]
    assert not bad, (row, bad)


def _truth(gold, key):
    return gold[key + "32"].astype(np.float64) + gold[key + "_d"]


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("config", list(T.CONFIGS))
def test_twelve_steps_against_the_record(gold, runs, config):
    _, opt, steps = runs[config]
    sizes, n_bn = gold["sizes"], int(gold["n_bn"])
    clipped = 0
    for t, s in enumerate(steps):
        assert (s["lr"], s["mom"], s["step"]) == (gold[f"{config}/lr"][t], gold[f"{config}/mom"][t], t + 1), t
        if gold[f"{config}/norm64"][t] > T.MAX_NORM:
            clipped += 1
            assert not np.array_equal(s["g"], s["fed"])
            assert abs(np.sqrt((s["g"].astype(np.float64) ** 2).sum()) - T.MAX_NORM) < 1e-4 * T.MAX_NORM
        else:                                   # a coefficient of 1 leaves the bits alone
            assert np.array_equal(s["g"].view(np.int32), s["fed"].view(np.int32)), t
    assert clipped * 3 == T.STEPS
    # the norm, over the twelve steps: errors relative to the norm itself
    n64 = gold[f"{config}/norm64"]
    _hold(f"{config}/norm", np.array([s["norm"] for s in steps]) / n64, gold[f"{config}/norm32"] / n64, np.ones(T.STEPS), [T.STEPS])
    last = steps[-1]
    if config == "tt":
        for k in "pmv":
            _hold(f"tt/{k}", last[k], gold[f"tt/{k}32"], _truth(gold, f"tt/{k}"), sizes)
    elif config == "tf":                        # the BatchNorm parameters are the record's; everything else is tt's, to the bit
        bn0 = T.offsets(sizes)[len(sizes) - n_bn]
        _hold("tf/p_bn", last["p"][bn0:], gold["tf/p32"], _truth(gold, "tf/p"), sizes[len(sizes) - n_bn:])
        tt = runs["tt"][2][-1]
        assert np.array_equal(last["p"][:bn0], tt["p"][:bn0]) and not np.array_equal(last["p"][bn0:], tt["p"][bn0:])
        assert np.array_equal(last["m"], tt["m"]) and np.array_equal(last["v"], tt["v"])
    else:
        _hold("cp/p", last["p"], gold["cp/p32"], _truth(gold, "cp/p"), sizes)
        # the coupled decay reaches the moments: against the restatement (float64 the truth, float32 the yardstick), which
        # tests/test_solver_cpu.py ties to the record at every step
        grad_fn = lambda t: T.grads_of(gold, t)
        r64 = T.run("cp", gold["init"], sizes, n_bn, grad_fn, torch.float64)[-1]
        r32 = T.run("cp", gold["init"], sizes, n_bn, grad_fn, torch.float32)[-1]
        for k in "mv":
            _hold(f"cp/{k}", last[k], r32[k], r64[k], sizes)
        assert not np.array_equal(last["m"], runs["tt"][2][-1]["m"])


def test_every_tensor_size_is_covered_and_the_pads_stay_zero(gold, runs):
    sizes = [int(s) for s in gold["sizes"]]
    assert {1, 3, 4095, 4096, 4097, 2 * 4096 + 5} <= set(sizes)
    off = T.offsets(sizes)
    for config, (_, opt, steps) in runs.items():
        _pads_are_zero(opt)
        assert opt._n_chunks == sum(-(-s // hip.OPTIM_CHUNK) for s in sizes) == len(sizes) + 3
        first, last = steps[0], steps[-1]
        truth = T.run(config, gold["init"], sizes, int(gold["n_bn"]), lambda t: T.grads_of(gold, t), torch.float64, steps=1)[0]
        for i in range(len(sizes)):             # every element of every tensor has moved, up to the tensor's last one
            sl = slice(off[i], off[i + 1])
            assert (last["p"][sl] != gold["init"][sl]).all(), (config, i)
            assert (last["v"][sl] > 0).all() and np.isfinite(last["p"][sl]).all(), (config, i)
            # one element wrong at a seam would stand out of its tensor's error
            d = np.abs(first["p"][sl] - truth["p"][sl])
            assert d.max() <= 1e-6 * max(np.abs(truth["p"][sl]).max(), 1e-3), (config, i, d.max())


# ------------------------------------------------------------------------------------------------ non-finite gradients
def _pattern(a):
    return np.isnan(a), np.isposinf(a), np.isneginf(a), a == 0


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("config", ["tt", "cp"])
@pytest.mark.parametrize("what", ["inf", "nan", "both"])
def test_non_finite_gradients_poison_what_they_poison_in_torch(gold, what, config, clip):
    sizes, n_bn = gold["sizes"], int(gold["n_bn"])
    off = T.offsets(sizes)
    i_big, i_tail = int(np.argmax(sizes)), list(sizes).index(4097)

    def grad_fn(t):
        g = T.grads_of(gold, t).copy()
        if t == 1:
            if what in ("inf", "both"):
                g[off[i_big] + 5000] = -np.inf          # the second chunk of the largest tensor
            if what in ("nan", "both"):
                g[off[i_tail] + 4096] = np.nan          # the one-element tail chunk
        return g
    want = T.run(config, gold["init"], sizes, n_bn, grad_fn, torch.float32, steps=3, max_norm=T.MAX_NORM if clip else None)
    _, opt, sched = _make(gold, config)
    sched.attach()
    opt.max_norm = T.MAX_NORM if clip else None
    for t in range(3):
        opt.zero_grad()
        _feed(opt, grad_fn(t))
        opt.step()
        got = _state(opt)
        for k in "pmvg":
            for a, b in zip(_pattern(got[k]), _pattern(want[t][k])):
                assert np.array_equal(a, b), (t, k, int((a != b).sum()))
        if t == 1:
            n = float(opt.total_norm())
            assert (np.isnan(n) if what != "inf" else np.isposinf(n)) and (np.isnan(want[t]["norm"]) if what != "inf" else np.isposinf(want[t]["norm"]))
    assert np.isnan(got["p"]).any()
    if not clip and what == "inf" and config == "tt":      # (coupled decay feeds the NaN parameter back into the moments)
        assert np.isnan(got["p"]).sum() == 1 and np.isposinf(got["v"]).sum() == 1
    _pads_are_zero(opt)


# ------------------------------------------------------------------------------------------------ reproducibility, routes
def test_two_runs_and_both_routes_give_identical_bits(gold, runs):
    _, _, a = runs["tt"]
    for route in ("table", "host"):
        _, _, b = _run(gold, "tt", route)
        for t in range(T.STEPS):
            assert a[t]["norm"] == b[t]["norm"] and (a[t]["lr"], a[t]["mom"], a[t]["step"]) == (b[t]["lr"], b[t]["mom"], b[t]["step"])
            for k in "pmvg":
                assert np.array_equal(a[t][k].view(np.int32), b[t][k].view(np.int32)), (route, t, k)


def test_without_clip_or_decay_and_fused_zero(gold):
    """no clip armed: the gradients are not touched at all; wd = 0 and bn_wd = False decay nothing; fused_zero leaves
    zeros and zero_grad() then launches nothing"""
    sizes, n_bn = gold["sizes"], int(gold["n_bn"])
    _, opt, sched = _make(gold, "tt", fused_zero=True)
    _, ref, sched_ref = _make(gold, "tt")
    for o, s in ((opt, sched), (ref, sched_ref)):
        s.attach()
    g = T.grads_of(gold, 1)
    for o in (opt, ref):
        o.zero_grad()
        _feed(o, g)
        o.step()
    a, b = _state(opt), _state(ref)
    assert not a["g"].any() and np.array_equal(b["g"].view(np.int32), g.view(np.int32))
    for k in "pmv":
        assert np.array_equal(a[k], b[k])
    want = T.run("tt", gold["init"], sizes, n_bn, lambda t: g, torch.float64, steps=1, max_norm=None)[0]
    f32 = T.run("tt", gold["init"], sizes, n_bn, lambda t: g, torch.float32, steps=1, max_norm=None)[0]
    for k in "pmv":
        _hold(f"noclip/{k}", a[k], f32[k], want[k], sizes)
    _pads_are_zero(opt)


# ------------------------------------------------------------------------------------------------ the captured graph
def test_captured_graph_walks_the_schedule_on_the_device(gold):
    def make():
        _, opt, sched = _make(gold, "tt", fused_zero=True)
        sched.attach()
        opt.max_norm = T.MAX_NORM
        return opt, torch.zeros(opt.n_flat, device="cuda")
    halves = []
    for t in range(6):
        buf = np.zeros(runs_n_flat(gold), np.float32)
        buf[runs_index(gold)] = T.grads_of(gold, t) / 2          # exact: the captured op doubles it
        halves.append(torch.from_numpy(buf).cuda())

    def iteration(opt, inp):
        torch.mul(inp, 2.0, out=opt._grad)                       # the "backward": one elementwise op into the flat buffer
        opt.step()

    eager, e_in = make()
    want = []
    for t in range(6):
        e_in.copy_(halves[t])
        iteration(eager, e_in)
        want.append(dict(lr=eager.lr, step=eager.step_count, **_state(eager)))

    cap, c_in = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c_in.copy_(halves[0])
        iteration(cap, c_in)                                     # iteration 0, eagerly on the side stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)                # the captured graph stays, to be walked below
    with torch.cuda.graph(graph, stream=side):
        iteration(cap, c_in)
    graph.instantiate()
    assert cap.step_count == 1                                   # the capture itself ran nothing
    lrs = []
    for t in range(1, 6):
        c_in.copy_(halves[t])
        graph.replay()
        got = dict(lr=cap.lr, step=cap.step_count, **_state(cap))
        lrs.append(got["lr"])
        assert (got["lr"], got["step"]) == (want[t]["lr"], want[t]["step"]) == (gold["tt/lr"][t], t + 1)
        for k in "pmvg":
            assert np.array_equal(got[k].view(np.int32), want[t][k].view(np.int32)), (t, k)
    assert len(set(lrs)) == 5                                    # a new row of the table at every replay
    # the graph is a straight chain: three kernels, no parallel branch
    n_nodes, edges = _graph_edges(graph)
    assert n_nodes == 3 and len(edges) == 2, (n_nodes, edges)
    nodes = {n for e in edges for n in e}
    assert len(nodes) == 3
    assert max(sum(1 for a, _ in edges if a == n) for n in nodes) == 1 and max(sum(1 for _, b in edges if b == n) for n in nodes) == 1


def _graph_edges(graph):
    """(node count, [(from, to)]) of a kept torch graph, asked of the HIP runtime that torch itself has loaded"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    rt = ctypes.CDLL(path)
    rt.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    rt.hipGraphGetEdges.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    raw = ctypes.c_void_p(int(graph.raw_cuda_graph()))
    n, ne = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert rt.hipGraphGetNodes(raw, None, ctypes.byref(n)) == 0
    assert rt.hipGraphGetEdges(raw, None, None, ctypes.byref(ne)) == 0
    src, dst = (ctypes.c_void_p * max(ne.value, 1))(), (ctypes.c_void_p * max(ne.value, 1))()
    assert rt.hipGraphGetEdges(raw, src, dst, ctypes.byref(ne)) == 0
    return n.value, [(src[i], dst[i]) for i in range(ne.value)]


def runs_n_flat(gold):
    return sum((int(s) + 3) // 4 * 4 for s in gold["sizes"])


def runs_index(gold):
    off, out = 0, []
    for s in gold["sizes"]:
        out.append(np.arange(off, off + int(s)))
        off += (int(s) + 3) // 4 * 4
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("through_torch", [False, True])
def test_resume_from_step_six_gives_the_uninterrupted_bits(gold, runs, through_torch):
    _, _, steps = runs["tt"]
    sd = steps[5]["sd"]
    assert set(sd["state"]) == set(range(len(gold["sizes"]))) and all(float(s["step"]) == 6 for s in sd["state"].values())
    model, opt, sched = _make(gold, "tt", init=steps[5]["p"])
    if through_torch:                           # the checkpoint goes through a stock torch.optim.Adam and comes back
        groups = [{"params": g} for g in opt._groups]
        adam = torch.optim.Adam(groups)
        adam.load_state_dict(sd)
        assert all(torch.equal(adam.state[p]["exp_avg"], opt_s["exp_avg"].cuda()) for p, opt_s in zip(opt.params, sd["state"].values()))
        sd = adam.state_dict()
    opt.load_state_dict(sd)
    assert opt.step_count == 6
    sched.attach()
    opt.max_norm = T.MAX_NORM
    for t in range(6, T.STEPS):
        opt.zero_grad()
        _feed(opt, T.grads_of(gold, t))
        opt.step()
        got = _state(opt)
        assert (opt.lr, opt.mom, opt.step_count) == (steps[t]["lr"], steps[t]["mom"], t + 1)
        for k in "pmvg":
            assert np.array_equal(got[k].view(np.int32), steps[t][k].view(np.int32)), (t, k)


def test_frozen_parameter_is_untouched_and_absent(gold, runs):
    for config, (model, opt, _) in runs.items():
        frozen = model.frozen.weight
        want = T.build_model(gold["init"], gold["names"]).frozen.weight
        assert torch.equal(frozen.cpu(), want) and frozen.grad is None and not frozen.requires_grad
        assert all(frozen is not p for p in opt.params)
        lo = frozen.data_ptr()
        assert all(not (r[0] < lo + 4 * frozen.numel() and lo < r[0] + 4 * r[2]) for r in opt.chunk_rows())


# ------------------------------------------------------------------------------------------------ the detector
def test_one_train_iter_of_the_small_voxelnet():
    V = importlib.import_module("test_gpu_voxelnet")
    detector, pillars = V.detector, V.pillars
    center_loss = importlib.import_module("3dal_pytorch_amd.center_loss")
    pts, off = V.sweep()
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    r = pillars.voxelize(dev(pts), off, V.VOXEL, V.RANGE, 5, 4000)
    voxels, coords, num, nv = r.finish()
    gt = np.zeros((2, 4, 10), np.float32)
    gt[0, 0] = [-1.5, 1.0, 0.0, 1.8, 4.2, 1.6, 0.3, 0, 0, 1]
    gt[0, 1] = [2.0, -2.5, 0.2, 0.7, 0.8, 1.7, -1.0, 0, 0, 2]
    gt[1, 0] = [0.5, 2.5, -0.1, 0.6, 1.7, 1.5, 2.0, 0, 0, 3]
    targets = center_loss.center_targets(dev(gt), [3], V.RANGE, V.VOXEL, 8, (2, 2))
    example = dict(voxels=voxels, coordinates=coords, num_points=num, num_voxels=nv, shape=[V.GRID] * 2, **targets)
    m = detector.VoxelNet(**V.MODEL, **V.KW)
    m.load_state_dict(V.checkpoint(), strict=True)
    m = m.cuda().train()
    opt = solver.OptimWrapper.create(ADAM, T.LR0, solver.get_layer_groups(m), wd=T.WD, true_wd=True, bn_wd=True)
    trainable = [p for p in m.parameters() if p.requires_grad]
    assert {id(p) for p in opt.params} == {id(p) for p in trainable}        # every parameter sits on a leaf module
    sched = solver.OneCycle(opt, T.TOTAL_STEP, T.ONE_CYCLE["lr_max"], T.ONE_CYCLE["moms"], T.ONE_CYCLE["div_factor"], T.ONE_CYCLE["pct_start"])
    sched.step(0)
    before = T.flat(opt.params)
    kept, inner = {}, opt.step

    def spy():                                  # the gradients as the step finds them
        kept["g"] = opt._grad.cpu().numpy()[_index(opt)]
        inner()
    opt.step = spy
    loss = sum(m.first_stage_loss(example)["loss"])
    solver.train_iter(opt, loss, grad_clip=CLIP)
    g = kept["g"]
    assert np.isfinite(g).all() and np.abs(g).max() > 0 and opt.step_count == 1
    sizes = [p.numel() for p in opt.params]
    n_bn = len(opt._groups[1])
    assert n_bn > 0
    r64 = T.run("tt", before, sizes, n_bn, lambda t: g, torch.float64, steps=1)[0]
    r32 = T.run("tt", before, sizes, n_bn, lambda t: g, torch.float32, steps=1)[0]
    got = _state(opt)
    norm = float(opt.total_norm())
    assert abs(norm - r64["norm"]) <= 1e-6 * r64["norm"]
    print(f"voxelnet: {len(sizes)} tensors, {sum(sizes)} elements, {opt._n_chunks} chunks, norm {norm:.4f}")
    for k in "pmv":
        _hold(f"voxelnet/{k}", got[k], r32[k], r64[k], sizes)
    assert (got["p"] != before).mean() > 0.99
