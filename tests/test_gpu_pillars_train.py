"""The pillar reader's training step on the GPU (PillarFeatureNet.train_forward / train_forward_canvas): outputs, the three
parameter gradients per layer and the running statistics against the float64 truth of tests/pillars_train_ref.py under its
BARS, with the torch-CPU fp32 composite as the yardstick; dead capacity rows, the fused canvas route, determinism, and
the reference's recorded step. DAL3_PILLARS_TRAIN_RECORD=<path> writes every measured / yardstick / ratio row (how
profiles/pillars_train_measured.json is made)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import pillars_ref as R
import pillars_train_ref as T

pillars = importlib.import_module("3dal_pytorch_amd.pillars")
pytestmark = pytest.mark.gpu
_RECORD = {}
GRID = [32, 32]                                             # PILLAR's nx, ny


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    path = os.environ.get("DAL3_PILLARS_TRAIN_RECORD")
    if path and _RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _step(n_layers, C, vox, num, co, cot, n_pillars=None, canvas_B=None, layout=None, max_workgroups=0):
    """one training step of a fresh module on the GPU -> (flat() rows as host arrays, the output tensor). cot: (P, 64), or the
    canvas cotangent with canvas_B; layout "channels_last" hands the backward that memory format."""
    net = T.module(n_layers, C).cuda()
    args = (_dev(vox), _dev(num), _dev(co))
    n_pillars = None if n_pillars is None else torch.tensor([n_pillars], dtype=torch.int64, device="cuda")
    if canvas_B is None:
        out = net.train_forward(*args, n_pillars=n_pillars, max_workgroups=max_workgroups)
    else:
        out = net.train_forward_canvas(*args, canvas_B, GRID, n_pillars=n_pillars, max_workgroups=max_workgroups)
    g = _dev(cot)
    if layout == "channels_last":
        g = g.contiguous(memory_format=torch.channels_last)
        assert not g.is_contiguous()
    out.backward(g)
    L = net.pfn_layers
    assert all(int(l.norm.num_batches_tracked) == 8 for l in L)         # reader_weights starts them at 7
    res = {"out": out.detach().cpu().numpy(), "dW": [l.linear.weight.grad.cpu().numpy() for l in L],
           "dgamma": [l.norm.weight.grad.cpu().numpy() for l in L], "dbeta": [l.norm.bias.grad.cpu().numpy() for l in L],
           "running_mean": [l.norm.running_mean.cpu().numpy() for l in L], "running_var": [l.norm.running_var.cpu().numpy() for l in L]}
    if canvas_B is not None:
        canvas = res.pop("out")
        rows = T.flat(dict(res, out=np.zeros((1, 64), np.float32)))
        rows["out"] = canvas
        return rows
    return T.flat(res)


def _same_bits(a, b, skip=()):
    assert set(a) == set(b)
    for row in a:
        if row not in skip:
            assert a[row].shape == b[row].shape and np.array_equal(a[row].view(np.uint32), b[row].view(np.uint32)), row


def _hold(name, got, f32, truth):
    bad = []
    for row, (ratio, m, y) in T.ratios(got, f32, truth).items():
        assert np.isfinite(got[row]).all(), (name, row)
        _RECORD[f"{name}/{row}"] = {"measured": {k: m[k] for k in R.MEASURES}, "yardstick": {k: y[k] for k in R.MEASURES}, "ratio": ratio}
        for k in R.MEASURES:
            print(f"{name + '/' + row:32s} {k:9s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:7.2f}  bar {T.BARS[k]:g}")
        bad += [(row, k, m[k], ratio[k]) for k in R.MEASURES if ratio[k] > T.BARS[k]]
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_step_against_float64(name):
    n_layers, C, _, _ = T.CASES[name]
    _, vox, num, co, cot, _ = T.case(name)
    truth, f32 = T.references(name)
    _hold(name, _step(n_layers, C, vox, num, co, cot), f32, truth)


def test_golden_record():
    vox, num, co, cot, _ = T.golden_inputs()
    for n_layers in (1, 2):
        _hold(f"golden/l{n_layers}", _step(n_layers, 5, vox, num, co, cot), T.golden_record(n_layers, "f32"),
              T.golden_record(n_layers, "f64"))


@pytest.mark.parametrize("n_layers", (1, 2))
def test_dead_capacity_rows(n_layers):
    """n_pillars < P, the dead rows' voxels NaN and their num_points and coordinates garbage: everything is finite and
    equals the run on the sliced live rows bit for bit; the dead rows of the output are zero"""
    name = f"l{n_layers}/P{T.SLICE + 1}"  if n_layers == 2 else f"l1/P{2 * T.SLICE + 3}"
    _, vox, num, co, cot, _ = T.case(name)
    P, dead = vox.shape[0], 77
    live = _step(n_layers, 5, vox, num, co, cot)
    vox2 = np.concatenate([vox, np.full((dead,) + vox.shape[1:], np.nan, np.float32)])
    num2 = np.concatenate([num, np.array([0, -7, 1000, 2 ** 31 - 1] * dead, np.int32)[:dead]])
    co2 = np.concatenate([co, np.full((dead, 4), -12345, np.int32)])
    cot2 = np.concatenate([cot, np.full((dead, 64), np.nan, np.float32)])
    got = _step(n_layers, 5, vox2, num2, co2, cot2, n_pillars=P)
    assert all(np.isfinite(v).all() for v in got.values())
    assert not got["out"][P:].any()
    got["out"] = got["out"][:P]
    _same_bits(got, live)
    # a count beyond the capacity is the capacity
    _same_bits(_step(n_layers, 5, vox, num, co, cot, n_pillars=P + 5), live)


@pytest.mark.parametrize("n_layers", (1, 2))
def test_canvas_route(n_layers):
    name = f"l{n_layers}/c5"
    _, vox, num, co, cot, _ = T.case(name, 2)
    assert set(co[:, 0].tolist()) == {0, 1}
    co = co.copy()
    co[5, 2] = GRID[1]                                      # one pillar outside the canvas: nothing written, no cotangent
    co[6, 0] = 2
    inside = np.ones(len(co), bool)
    inside[[5, 6]] = False
    P = vox.shape[0]
    gc = T.synth.normal(R.SEED, "pillars_train/canvas_cot", (2, 64, GRID[1], GRID[0]), 0.0, 1.0).astype(np.float32)
    a = _step(n_layers, 5, vox, num, co, gc, canvas_B=2)
    b = _step(n_layers, 5, vox, num, co, gc, canvas_B=2, layout="channels_last")
    _same_bits(a, b)
    # the canvas is train_forward + PointPillarsScatter, and the gradients those of the cotangent read at the pillars' cells
    rows = np.where(inside[:, None], gc[np.minimum(co[:, 0], 1), :, np.minimum(co[:, 2], GRID[1] - 1), co[:, 3]], 0).astype(np.float32)
    f = _step(n_layers, 5, vox, num, co, rows)
    want = pillars.PointPillarsScatter(64)(_dev(f["out"]), _dev(co), 2, GRID).cpu().numpy()
    assert np.array_equal(a["out"].view(np.uint32), want.view(np.uint32))
    assert a["out"].any()
    _same_bits(a, f, skip=("out",))
    # a sliced cotangent (every other channel's storage skipped) is read through its strides too
    wide = torch.zeros((2, 128, GRID[1], GRID[0]), device="cuda")
    wide[:, ::2] = _dev(gc)
    net = T.module(n_layers, 5).cuda()
    out = net.train_forward_canvas(_dev(vox), _dev(num), _dev(co), 2, GRID)
    out.backward(wide[:, ::2])
    for i, l in enumerate(net.pfn_layers):
        assert np.array_equal(l.linear.weight.grad.cpu().numpy().T.view(np.uint32), a[f"dW{i + 1}"].view(np.uint32))


@pytest.mark.parametrize("name", (f"l2/P{2 * T.SLICE + 3}", f"l1/P{2 * T.SLICE + 3}", "l2/rows64"))
def test_determinism(name):
    n_layers, C, _, _ = T.CASES[name]
    _, vox, num, co, cot, _ = T.case(name)
    first = _step(n_layers, C, vox, num, co, cot)
    _same_bits(_step(n_layers, C, vox, num, co, cot), first)
    for cap in (1, 3):
        _same_bits(_step(n_layers, C, vox, num, co, cot, max_workgroups=cap), first)


def test_refusals():
    _, vox, num, co, _, _ = T.case("l2/c5")
    args = (_dev(vox), _dev(num), _dev(co))
    net = T.module(2, 5).cuda()
    with pytest.raises(RuntimeError, match="eval mode"):
        net.eval().train_forward(*args)
    with pytest.raises(RuntimeError, match="hip_serves"):
        T.module(2, 5).cuda().train_forward(_dev(vox[:, :, :4]), *args[1:])
    wide = pillars.PillarFeatureNet(num_input_features=5, num_filters=(32, 64)).cuda().train()
    with pytest.raises(RuntimeError, match="hip_serves"):
        wide.train_forward_canvas(*args, 1, GRID)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        T.module(1, 5).cuda().train_forward(_dev(vox[:1, :1]), _dev(num[:1]), _dev(co[:1]))
    # forward() in train mode stays the composite, and eval mode works after a training step (the pack is rebuilt)
    net = T.module(2, 5).cuda()
    net.train_forward(*args).sum().backward()
    ref = T.module(2, 5).cuda()
    ref.composite(*args)
    for l, m in zip(net.pfn_layers, ref.pfn_layers):
        assert torch.allclose(l.norm.running_var, m.norm.running_var, rtol=1e-5)
    assert torch.allclose(net.eval()(*args), ref.eval()(*args), rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------- the detector
# The loss test's grid: 12 x 12 pillars of 0.32 m, B = 2 (about 260 pillars, three slices). It is this small because the
# neck and the head decide a ReLU per activation and no search can keep them all away from 0: on test_gpu_detector's
# 44 x 36 grid they are 4 x 10^6 decisions and a few flip between any two fp32 evaluations, which moves a gradient by
# 1e-3 whoever computes it; here they are 3 x 10^5.
VOXEL, RANGE, SHAPE = (0.32, 0.32, 6.0), (0.0, -1.92, -2.0, 3.84, 1.92, 4.0), [12, 12, 1]


def _detector_case():
    D = importlib.import_module("test_gpu_detector")
    center_loss = importlib.import_module("3dal_pytorch_amd.center_loss")
    pts, off, _ = T.detector_sweep(VOXEL, RANGE)
    r = pillars.voxelize(_dev(pts), off, VOXEL, RANGE, 20, 2000)
    gt = np.zeros((2, 4, 10), np.float32)
    gt[0, 0] = [1.0, 0.5, 0.0, 1.8, 4.2, 1.6, 0.3, 0, 0, 1]
    gt[0, 1] = [2.8, -1.0, 0.2, 0.7, 0.8, 1.7, -1.0, 0, 0, 2]
    gt[1, 0] = [2.0, 1.0, -0.1, 0.6, 1.7, 1.5, 2.0, 0, 0, 3]
    targets = center_loss.center_targets(_dev(gt), [3], RANGE, VOXEL, 1, (SHAPE[1], SHAPE[0]))
    return D, r, targets


def _detector(D, device="cuda", small=True):
    model = dict(D.MODEL, reader=dict(D.MODEL["reader"], voxel_size=VOXEL, pc_range=RANGE)) if small else D.MODEL
    m = D.detector.PointPillars(**model, max_points=20, max_voxels=2000)
    m.load_state_dict(D.checkpoint(), strict=True)
    return m.to(device).train()


def _cat(preds):
    return torch.cat([v for d in preds for v in d.values()], 1)


def _rows_of(m, maps):
    """what a step leaves: the head's maps, every parameter's gradient, every running statistic -> {row: array}"""
    rows = {"maps": maps.detach().cpu().numpy()}
    rows.update({"grad/" + k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()})
    rows.update({"stat/" + k: v.detach().cpu().numpy() for k, v in m.named_buffers() if not k.endswith("num_batches_tracked")})
    return rows


def _loss_run(D, example, reader):
    """one first_stage_loss + backward on a fresh model -> (loss, the canvas, the rows, d loss / d maps)"""
    m = _detector(D)
    kept, neck, head = {}, m.neck.composite, m.bbox_head.composite

    def spy_neck(x):
        kept["canvas"] = x
        return neck(x)

    def spy_head(x):
        kept["preds"] = head(x)
        for d in kept["preds"]:
            for v in d.values():
                v.retain_grad()
        return kept["preds"]
    m.neck.composite, m.bbox_head.composite = spy_neck, spy_head
    out = m.first_stage_loss(example, reader=reader)
    loss = sum(out["loss"])
    loss.backward()
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0 and float(out["num_positive"][0]) > 0
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (reader, k)
    cot = torch.cat([v.grad for d in kept["preds"] for v in d.values()], 1).cpu().numpy()
    return loss.detach(), kept["canvas"].detach(), _rows_of(m, _cat(kept["preds"])), cot


def _cpu_chain(D, vox, num, co, cot, dtype):
    """reader.composite -> scatter -> neck.composite -> head.composite on the CPU in `dtype` under the head's cotangent"""
    m = _detector(D, "cpu").to(dtype)
    with torch.enable_grad():
        feats = m.reader.composite(torch.from_numpy(vox).to(dtype), torch.from_numpy(num), torch.from_numpy(co))
        at = torch.from_numpy(co).long()
        canvas = feats.new_zeros((2, 64, SHAPE[1], SHAPE[0]))
        canvas[at[:, 0], :, at[:, 2], at[:, 3]] = feats
        maps = _cat(m.bbox_head.composite(m.neck.composite(canvas)))
        maps.backward(torch.from_numpy(cot).to(dtype))
    return _rows_of(m, maps)


def _tensor_error(got, truth):
    return float(np.abs(got.astype(np.float64) - truth).max() / np.abs(truth).max())


def test_first_stage_loss_reader_routes():
    """`loss` and every parameter's gradient, reader="hip" against reader="composite", on a 12 x 12 grid with B = 2 and
    the seeded checkpoint. CenterHead.loss runs only on the GPU, so each route's d loss / d maps is taken from the GPU
    and the whole chain behind it (reader, scatter, neck, head: the composites) is run on the CPU in float64, the truth,
    and in float32, the yardstick, under that cotangent. By tensor, under BARS: (a) every row of each route against the
    truth with the CPU fp32 chain as the yardstick; (b) the hip route's error against the composite route's own error,
    the same stock-torch fp32 chain on the same device, row by row. (c) The two losses: the loss is a function of the
    maps, so to first order they differ by <d loss / d maps, maps_hip - maps_composite>, taken in float64 here; the bound
    is twice that plus 64 eps of the loss for the rounding of two fp32 sums over about 10^4 terms. The sweep keeps the
    reader's decisions MARGIN away from a flip (pillars_train_ref.detector_sweep)."""
    rpn_train = importlib.import_module("rpn_train_ref")
    D, r, targets = _detector_case()
    voxels, coords, num, nv = r.finish()
    example = dict(voxels=voxels, coordinates=coords, num_points=num, num_voxels=nv, shape=[SHAPE] * 2, **targets)
    capacity = dict(example, voxels=r.voxels, coordinates=r.coordinates, num_points=r.num_points, n_voxels=r.n_pillars)
    assert r.voxels.shape[0] > voxels.shape[0] and set(coords[:, 0].tolist()) == {0, 1}
    with pytest.raises(ValueError, match="n_voxels"):
        _detector(D).first_stage_loss(capacity, reader="composite")
    with pytest.raises(ValueError, match="reader"):
        _detector(D).first_stage_loss(example, reader="triton")
    hip, comp, cap = _loss_run(D, example, "hip"), _loss_run(D, example, "composite"), _loss_run(D, capacity, "hip")
    # the capacity-sized example with its device count: the canvas has the sliced one's bits (the stock-torch neck and
    # head behind it do not promise theirs from run to run)
    assert torch.equal(cap[1], hip[1])
    vox, n, co = voxels.cpu().numpy(), num.cpu().numpy(), coords.cpu().numpy()
    fresh = _detector(D, "cpu")
    zero = {f"grad/{name}.{k}" for name, mod in (("neck", fresh.neck), ("bbox_head", fresh.bbox_head)) for k in rpn_train.zero_by_batchnorm(mod)}
    errors = {}
    for route, (loss, canvas, got, cot) in (("hip", hip), ("composite", comp)):
        assert np.abs(cot).max() > 0
        truth, f32 = _cpu_chain(D, vox, n, co, cot, torch.float64), _cpu_chain(D, vox, n, co, cot, torch.float32)
        assert set(got) == set(truth)
        bad = []
        for row in sorted(truth):
            if row in zero:                                 # a bias in front of a train-mode BatchNorm: the true gradient is 0
                assert np.abs(got[row]).max() <= 1e-4 * np.abs(truth[row.replace(".bias", ".weight")]).max(), row
                continue
            e, y = _tensor_error(got[row], truth[row]), max(_tensor_error(f32[row], truth[row]), R.FLOOR)
            errors[route, row] = e
            _RECORD[f"first_stage/{route}/{row}"] = {"measured": {"tensor": e}, "yardstick": {"tensor": y}, "ratio": {"tensor": e / y}}
            print(f"first_stage/{route}/{row:52s} tensor {e:10.3e}  yardstick {y:10.3e}  ratio {e / y:7.2f}")
            bad += [(row, e, e / y)] if e > T.BARS["tensor"] * y else []
        assert not bad, (route, bad)
    rows = sorted(row for route, row in errors if route == "hip")
    assert any(row.startswith("grad/reader.") for row in rows) and any(row.startswith("grad/neck.") for row in rows) and \
        any(row.startswith("grad/bbox_head.") for row in rows)
    bad = []
    for row in rows:
        e, y = errors["hip", row], max(errors["composite", row], R.FLOOR)
        _RECORD[f"first_stage/hip_over_composite/{row}"] = {"measured": {"tensor": e}, "yardstick": {"tensor": y}, "ratio": {"tensor": e / y}}
        bad += [(row, e, e / y)] if e > T.BARS["tensor"] * y else []
    assert not bad, bad
    first_order = abs(float((comp[3].astype(np.float64) * (hip[2]["maps"].astype(np.float64) - comp[2]["maps"])).sum()))
    diff, scale = abs(float(hip[0]) - float(comp[0])), abs(float(comp[0]))
    print(f"loss hip {float(hip[0]):.7f} composite {float(comp[0]):.7f}  |diff| {diff:.3e}  first order {first_order:.3e}")
    assert diff <= 2 * first_order + 64 * float(np.finfo(np.float32).eps) * scale


class _SyncCount:
    """counts the Python-level calls that wait for the device: torch.cuda.synchronize, Stream / Event.synchronize and, on a
    CUDA tensor, item / cpu / tolist / numpy / to(a CPU target) / nonzero / bool() / float() / int() / index use, and
    torch.nonzero. A read-back made inside a C++ operator without one of these (a boolean-mask index, for one) is outside
    what it sees."""
    METHODS = ("item", "cpu", "tolist", "numpy", "nonzero", "__bool__", "__float__", "__int__", "__index__")

    def __init__(self):
        self.calls = []

    def _wrap(self, owner, name, hit):
        fn = getattr(owner, name)
        self.saved.append((owner, name, fn))

        def counted(*a, **k):
            if hit(a, k):
                self.calls.append(name)
            return fn(*a, **k)
        setattr(owner, name, counted)

    def __enter__(self):
        self.saved = []
        always = lambda a, k: True
        on_cuda = lambda a, k: bool(a) and torch.is_tensor(a[0]) and a[0].is_cuda
        for owner in (torch.cuda, torch.cuda.Stream, torch.cuda.Event):
            self._wrap(owner, "synchronize", always)
        for name in self.METHODS:
            self._wrap(torch.Tensor, name, on_cuda)
        self._wrap(torch, "nonzero", on_cuda)

        def to_host(a, k):
            target = [x for x in list(a[1:]) + list(k.values()) if isinstance(x, (str, torch.device))]
            return on_cuda(a, k) and any(torch.device(x).type == "cpu" for x in target)
        self._wrap(torch.Tensor, "to", to_host)
        return self

    def __exit__(self, *exc):
        for owner, name, fn in reversed(self.saved):
            setattr(owner, name, fn)


def test_train_step_from_sweeps_and_train_iter_without_a_synchronisation():
    D, _, _ = _detector_case()
    augment = importlib.import_module("3dal_pytorch_amd.augment")
    center_loss = importlib.import_module("3dal_pytorch_amd.center_loss")
    solver = importlib.import_module("3dal_pytorch_amd.solver")
    import functools
    pts, off = D.sweep()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    cfg = dict(mode="train", shuffle_points=True, global_rot_noise=0.2, global_scale_noise=[0.95, 1.05], global_translate_std=0.1,
               class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"], db_sampler=None)
    pre = augment.Preprocess(cfg, pc_range=D.RANGE, max_objs=32, generator=gen)
    acfg = dict(out_size_factor=1, target_assigner=dict(tasks=[dict(num_class=3, class_names=cfg["class_names"])]),
                gaussian_overlap=0.1, max_objs=32, min_radius=2)
    m = _detector(D, small=False)
    with pytest.raises(RuntimeError, match="set_train_input"):
        m.train_step_from_sweeps(None, None, {})
    m.set_train_input(pre, center_loss.AssignLabel(cfg=acfg))
    gt = np.zeros((2, 2, 9), np.float32)
    gt[0, 0] = [3.5, 1.0, 0.0, 1.8, 4.2, 1.6, 0.5, 0.1, 0.3]
    gt[0, 1] = [9.0, -2.5, 0.2, 0.7, 0.8, 1.7, 0, 0, -1.0]
    gt[1, 0] = [6.5, 2.5, -0.1, 0.6, 1.7, 1.5, 0, 0, 2.0]
    ann = dict(gt_boxes=_dev(gt), gt_classes=np.array([[1, 2], [3, 0]], np.int32), gt_counts=np.array([2, 1], np.int32))
    adam = functools.partial(torch.optim.Adam, betas=(0.9, 0.99), amsgrad=0.0)
    opt = solver.OptimWrapper.create(adam, 3e-3, solver.get_layer_groups(m), wd=0.01, true_wd=True, bn_wd=True)
    assert {id(p) for p in opt.params} == {id(p) for p in m.parameters() if p.requires_grad}
    dpts = _dev(pts)
    # the first step loads the library, builds the optimiser's tables and warms the allocator
    solver.train_iter(opt, sum(m.train_step_from_sweeps(dpts, off, ann)["loss"]), grad_clip=dict(max_norm=35, norm_type=2))
    before = [p.detach().clone() for p in m.parameters()]
    torch.cuda.synchronize()
    with _SyncCount() as count:
        out = m.train_step_from_sweeps(dpts, off, ann, reader="hip")
        loss = sum(out["loss"])
        solver.train_iter(opt, loss, grad_clip=dict(max_norm=35, norm_type=2))
    assert count.calls == [], count.calls
    assert all(bool(torch.isfinite(v).all()) for k in ("loss", "hm_loss", "loc_loss") for v in out[k])
    assert int(m.last_example["augment_status"].item()) == 0 and int(m.last_example["voxel_status"].item()) == 0
    for (k, p), b in zip(m.named_parameters(), before):
        assert bool(torch.isfinite(p).all()) and bool((p != b).any()), k
