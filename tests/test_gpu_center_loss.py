"""The first stage's targets and loss on the GPU (3dal_pytorch_amd/center_loss.py, rpn.CenterHead.loss; dal3_center_targets,
dal3_center_loss) against the reference's own record (tests/golden/center_loss.npz): discrete outputs exactly, copied
outputs bit for bit, the heat map within one float32 ulp, floating outputs in multiples of the reference's fp32 error
against float64 (center_ref.BARS); both map layouts, reproducibility, the chained call, non-finite inputs, the overflow
bit, the many-block reduction at 188 x 188 and a small head end to end. DAL3_CENTER_LOSS_RECORD=<path> writes every figure
held (how profiles/center_loss_measured.json is made)."""
import copy
import importlib
import json
import os

import numpy as np
import pytest
import torch

import center_ref as T
from _common import golden
from test_center_loss_cpu import TARGET_KEYS, recorded_targets

hip = importlib.import_module("3dal_pytorch_amd._hip")
rpn = importlib.import_module("3dal_pytorch_amd.rpn")
center_loss = importlib.import_module("3dal_pytorch_amd.center_loss")
pytestmark = pytest.mark.gpu

_RECORD = {}
LOSS_KEYS = ("loss", "hm_loss", "loc_loss")
FUNCTION_COLS = [3, 4, 5, 8, 9]                 # log(w, l, h), sin, cos
COPIED_COLS = [0, 1, 2, 6, 7]                   # the offsets (exact differences), z, vx, vy


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    path = os.environ.get("DAL3_CENTER_LOSS_RECORD")
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
    return golden("center_loss")


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _pixels(a):
    """(B, C, H, W) -> (B * H * W, C): a map's channels are the measures' channels"""
    a = np.asarray(a)
    return a.transpose(0, 2, 3, 1).reshape(-1, a.shape[1])


def _hold(row, kind, got, f32, truth, structural_zeros=True):
    """each measure <= BARS[kind] x the reference's own fp32 error against float64. A channel that is 0 in the truth is +0
    where that zero is structural (a map's untouched channel). A parameter gradient can be 0 in float64 by exact
    cancellation of equal terms (+-coef over as many slots of either sign): there the float32 runs leave rounding
    residue, and the channel is held to BARS[kind] x the yardstick's own residue instead."""
    got, f32, truth = (np.asarray(a) for a in (got, f32, truth))
    ratio, m, y = T.ratios(got, f32, truth)
    _RECORD[row] = {"kind": kind, "measured": {k: m[k] for k in T.MEASURES}, "yardstick": {k: y[k] for k in T.MEASURES}, "ratio": ratio}
    for k in T.MEASURES:
        print(f"{row:44s} {k:9s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:9.2f}  bar {T.BARS[kind]:g}")
    if structural_zeros:
        assert m["dead_ok"], row
    else:
        zero = np.abs(truth).max(0) == 0
        assert np.abs(got[:, zero]).max(initial=0.0) <= T.BARS[kind] * np.abs(f32[:, zero]).max(initial=0.0), row
    bad = [(k, m[k], ratio[k]) for k in T.MEASURES if not ratio[k] <= T.BARS[kind]]
    assert not bad, (row, bad)


def _targets(gt, max_objs=16):
    a = center_loss.AssignLabel(cfg=dict(T.ASSIGNER, max_objs=max_objs), voxels=T.VOXELS)
    return a(_dev(gt))


def _ulps(got, want):
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def _check_targets(row, got, want):
    """got: center_targets' dictionary; want: the record's or the restatement's (with anno_box64)"""
    n_diff = 0
    for t in range(len(want["hm"])):
        g = {k: _np(got[k][t]) for k in TARGET_KEYS}
        for k in ("ind", "mask", "cat"):
            assert g[k].dtype == want[k][t].dtype and np.array_equal(g[k], want[k][t]), (row, t, k)
        assert g["hm"].dtype == np.float32 and g["anno_box"].dtype == np.float32
        assert np.array_equal(g["anno_box"][..., COPIED_COLS], want["anno_box"][t][..., COPIED_COLS]), (row, t)
        u = _ulps(g["hm"], want["hm"][t])
        assert u.max() <= 1, (row, t, int(u.max()))
        assert not g["hm"][want["hm"][t] == 0].any() and (g["hm"] >= 0).all() and (g["hm"] <= 1).all()
        b, k = np.nonzero(want["mask"][t])
        peak = g["hm"].reshape(g["hm"].shape[0], g["hm"].shape[1], -1)[b, want["cat"][t][b, k], want["ind"][t][b, k]]
        assert (peak == 1.0).all(), (row, t)
        n_diff += int((u > 0).sum())
        live = want["mask"][t] > 0
        if live.any():
            _hold(f"{row}/t{t}/anno_box", "anno_box", g["anno_box"][live][:, FUNCTION_COLS], want["anno_box"][t][live][:, FUNCTION_COLS],
                  want["anno_box64"][t][live][:, FUNCTION_COLS])
        assert not g["anno_box"][~live].any()
    _RECORD[f"{row}/hm_elements_one_ulp_off"] = n_diff
    print(f"{row}: {n_diff} heat-map elements one ulp from the reference")


def _split_maps(preds, sliced):
    """per task: the maps as leaves. sliced: channel slices of ONE leaf tensor per task (the kernel route's layout)"""
    out, leaves = [], []
    for p in preds:
        names = list(p)
        if sliced:
            whole = _dev(np.concatenate([p[h] for h in names], 1)).requires_grad_(True)
            parts = torch.split(whole, [p[h].shape[1] for h in names], dim=1)
            out.append(dict(zip(names, parts)))
            leaves.append((names, whole, [p[h].shape[1] for h in names]))
        else:
            d = {h: _dev(p[h]).requires_grad_(True) for h in names}
            out.append(d)
            leaves.append((names, d, None))
    return out, leaves


def _grads(leaves):
    out = []
    for names, leaf, widths in leaves:
        if widths is None:
            out.append({h: leaf[h].grad for h in names})
        else:
            out.append(dict(zip(names, torch.split(leaf.grad, widths, dim=1))))
    return out


def _head(code, tasks=T.TASKS):
    dataset, cw, weight, with_vel = T.CODES[code]
    return rpn.CenterHead(in_channels=16, tasks=tasks, dataset=dataset, weight=weight, code_weights=cw,
                          common_heads=T.HEADS9 if with_vel else T.HEADS7, share_conv_channel=64).cuda()


def _run_loss(head, preds, example, sliced=False):
    maps, leaves = _split_maps(preds, sliced)
    before = [{h: v.detach().clone() for h, v in m.items()} for m in maps]
    rets = head.loss(example, maps)
    sum(rets["loss"]).backward()
    for m, b in zip(maps, before):              # preds_dicts is not mutated
        assert set(m) == set(b) and all(torch.equal(m[h].detach().view(torch.int32), b[h].view(torch.int32)) for h in m)
    return rets, _grads(leaves)


def _example(tg):
    return {k: [_dev(v) for v in tg[k]] for k in TARGET_KEYS}


# ------------------------------------------------------------------------------------------------- targets
@pytest.mark.parametrize("tag", ["main", "empty"])
def test_targets_equal_the_reference_record(gold, tag):
    got = _targets(T.golden_gt(tag))
    assert int(got["status"].item()) == 0
    assert [got[k][0].dtype for k in TARGET_KEYS] == [torch.float32, torch.float32, torch.int64, torch.uint8, torch.int64]
    assert tuple(got["hm"][1].shape) == (2, 2, T.H, T.W) and tuple(got["anno_box"][0].shape) == (2, 16, 10)
    _check_targets(f"targets/{tag}", got, recorded_targets(gold, tag))


def test_targets_are_reproducible_and_skip_non_finite_rows():
    gt = T.golden_gt("main")
    a, b = _targets(gt), _targets(gt)
    clean = gt.copy()
    clean[0, 6:8] = 0                           # the NaN and the 1e20 row, the last two of task 0: no other row's k moves
    c = _targets(clean)
    for k in TARGET_KEYS:
        for t in range(2):
            assert torch.equal(a[k][t], b[k][t]) and torch.equal(a[k][t], c[k][t]), (k, t)
    assert torch.isfinite(a["hm"][0]).all() and torch.isfinite(a["anno_box"][0]).all()


def test_more_rows_than_max_objs_set_the_status_bit():
    gt = T.golden_gt("main")
    got = _targets(gt, max_objs=4)
    assert int(got["status"].item()) == hip.CENTER_OVERFLOW == 16384
    want = T.targets(gt, T.NUM_CLASSES, T.VOXELS, 8, (T.H, T.W), max_objs=4)
    _check_targets("targets/overflow", got, want)
    assert int(_targets(gt, max_objs=8)["status"].item()) == 0      # task 0 of sample 0 has exactly 8 rows


# ------------------------------------------------------------------------------------------------- the loss
def _check_loss(row, rets, grads, want32, want64, preds):
    for t in range(len(want64)):
        got = np.stack([_np(rets[k][t]) for k in LOSS_KEYS] + list(_np(rets["loc_loss_elem"][t])))
        f32 = np.stack([want32[t][k] for k in LOSS_KEYS] + list(want32[t]["loc_loss_elem"]))
        truth = np.stack([want64[t][k] for k in LOSS_KEYS] + list(want64[t]["loc_loss_elem"]))
        _hold(f"{row}/t{t}/loss", "loss", got[None], f32[None], truth[None])
        assert float(rets["num_positive"][t]) == float(want32[t]["num_positive"])
        assert all(rets[k][t].is_cuda and rets[k][t].dtype == torch.float32 for k in rets)
        assert rets["loss"][t].requires_grad and not rets["hm_loss"][t].requires_grad and not rets["loc_loss_elem"][t].requires_grad
        for h in preds[t]:
            _hold(f"{row}/t{t}/grad.{h}", "grad", _pixels(_np(grads[t][h])), _pixels(want32[t][f"grad.{h}"]), _pixels(want64[t][f"grad.{h}"]))
        # where the reference's clamp binds the gradient is exactly zero
        s = 1 / (1 + np.exp(-preds[t]["hm"].astype(np.float64)))
        bound = (s < 0.99e-4) | (s > 1 - 0.99e-4)
        assert not _np(grads[t]["hm"])[bound].any(), (row, t)


@pytest.mark.parametrize("tag", ["main", "empty"])
@pytest.mark.parametrize("code", ["c10", "c8"])
def test_loss_and_gradients_equal_the_reference_record(gold, tag, code):
    with_vel = T.CODES[code][3]
    tg = recorded_targets(gold, tag)
    preds = T.head_maps(f"{tag}/{code}", tg, T.NUM_CLASSES, with_vel)
    want32, want64 = [], []
    for t in range(2):
        names = ("loss", "hm_loss", "loc_loss", "loc_loss_elem", "num_positive") + tuple(f"grad.{h}" for h in preds[t])
        f32 = {n: gold[f"{tag}_{code}_t{t}_{n}_f32"] for n in names}
        want32.append(f32)
        want64.append({n: f32[n].astype(np.float64) + gold[f"{tag}_{code}_t{t}_{n}_diff"].astype(np.float64) for n in names})
    head, ex = _head(code), _example(tg)
    rets, grads = _run_loss(head, preds, ex)
    _check_loss(f"loss/{tag}/{code}", rets, grads, want32, want64, preds)
    # the kernel route's layout (channel slices of one tensor per task) and a second run: the same bits
    for sliced in (True, False):
        rets2, grads2 = _run_loss(head, preds, ex, sliced=sliced)
        for t in range(2):
            for k in rets:
                assert torch.equal(rets[k][t], rets2[k][t]), (sliced, k, t)
            for h in preds[t]:
                assert torch.equal(grads[t][h], grads2[t][h]), (sliced, h, t)
    if tag == "empty":
        assert float(rets["loc_loss"][1]) == 0 and float(rets["num_positive"][1]) == 0 and float(rets["hm_loss"][1]) > 0


def test_loss_from_gt_equals_targets_then_loss(gold):
    gt = _dev(T.golden_gt("main"))
    assigner = center_loss.AssignLabel(cfg=T.ASSIGNER, voxels=T.VOXELS)
    preds = T.head_maps("main/c10", recorded_targets(gold, "main"), T.NUM_CLASSES, True)
    head = _head("c10")
    maps, leaves = _split_maps(preds, False)
    chained = head.loss_from_gt(maps, gt, assigner)
    sum(chained["loss"]).backward()
    g1 = _grads(leaves)
    maps, leaves = _split_maps(preds, False)
    stepwise = head.loss(assigner(gt), maps)
    sum(stepwise["loss"]).backward()
    g2 = _grads(leaves)
    for t in range(2):
        for k in chained:
            assert torch.equal(chained[k][t], stepwise[k][t]), (k, t)
        for h in preds[t]:
            assert torch.equal(g1[t][h], g2[t][h]), (h, t)


def test_targets_that_are_not_contiguous_give_the_same_bits(gold):
    """ind and cat as interleaved views of one tensor (the same size: a freed copy of one is the block the other's copy
    gets), mask, anno_box and hm as strided views"""
    tg = recorded_targets(gold, "main")
    preds = T.head_maps("main/c10", tg, T.NUM_CLASSES, True)
    head, ex = _head("c10"), _example(tg)
    views = {k: [] for k in TARGET_KEYS}
    for t in range(2):
        both = torch.stack((ex["ind"][t], ex["cat"][t]), -1)
        views["ind"].append(both[..., 0])
        views["cat"].append(both[..., 1])
        for k in ("mask", "anno_box", "hm"):
            views[k].append(torch.stack((ex[k][t], torch.zeros_like(ex[k][t])), -1)[..., 0])
        assert not any(views[k][t].is_contiguous() for k in TARGET_KEYS)
    rets, grads = _run_loss(head, preds, ex)
    rets2, grads2 = _run_loss(head, preds, views)
    for t in range(2):
        assert all(torch.equal(rets[k][t], rets2[k][t]) for k in rets) and all(torch.equal(grads[t][h], grads2[t][h]) for h in preds[t])


def test_a_nan_logit_gives_a_nan_heat_map_loss_and_a_finite_location_loss(gold):
    tg = recorded_targets(gold, "main")
    preds = T.head_maps("main/c10", tg, T.NUM_CLASSES, True)
    preds[0]["hm"][1, 0, 3, 7] = np.nan
    rets, _ = _run_loss(_head("c10"), preds, _example(tg))
    assert torch.isnan(rets["hm_loss"][0]) and torch.isnan(rets["loss"][0]) and torch.isfinite(rets["loc_loss"][0])
    assert torch.isfinite(rets["loc_loss_elem"][0]).all() and torch.isfinite(rets["loss"][1])


def test_criteria_modules(gold):
    tg = recorded_targets(gold, "main")
    preds = T.head_maps("main/c8", tg, T.NUM_CLASSES, False)
    ex = _example(tg)
    rets, _ = _run_loss(_head("c8"), preds, ex)
    p = {h: _dev(v) for h, v in preds[1].items()}
    out = torch.clamp(torch.sigmoid(p["hm"]), min=1e-4, max=1 - 1e-4)
    hm_loss = center_loss.FastFocalLoss()(out, ex["hm"][1], ex["ind"][1], ex["mask"][1], ex["cat"][1])
    assert abs(float(hm_loss) - float(rets["hm_loss"][1])) <= 1e-5 * abs(float(rets["hm_loss"][1]))
    box = torch.cat([p[h] for h in ("reg", "height", "dim", "rot")], 1)
    elem = center_loss.RegLoss()(box, ex["mask"][1], ex["ind"][1], ex["anno_box"][1][..., [0, 1, 2, 3, 4, 5, 8, 9]])
    assert torch.equal(elem, rets["loc_loss_elem"][1])          # the Waymo weights are all 1


# ------------------------------------------------------------------------------------------------- the first real shape
@pytest.fixture(scope="module")
def mid():
    """188 x 188, B = 2, 3 classes, 500 slots, 60 objects a sample: the restatement, computed once"""
    m, gt = T.MID, T.mid_gt()
    tg = T.targets(gt, m["num_classes"], m["voxels"], m["out_size_factor"], (m["H"], m["W"]), max_objs=m["max_objs"])
    preds = T.head_maps("mid", tg, m["num_classes"], True, special=False)
    cw, weight = T.CODES["c10"][1], T.CODES["c10"][2]
    return gt, tg, preds, T.loss(preds, tg, cw, weight, T.F32), T.loss(preds, tg, cw, weight, T.F64)


def test_the_many_block_reduction_at_the_first_real_shape(mid):
    gt, tg, preds, want32, want64 = mid
    m = T.MID
    got = center_loss.center_targets(_dev(gt), m["num_classes"], m["voxels"]["range"], m["voxels"]["size"], m["out_size_factor"],
                                     (m["H"], m["W"]), max_objs=m["max_objs"])
    assert int(got["status"].item()) == 0
    _check_targets("targets/mid", got, tg)
    head = _head("c10", tasks=[dict(num_class=3, class_names=["a", "b", "c"])])
    rets, grads = _run_loss(head, preds, {k: got[k] for k in TARGET_KEYS})
    _check_loss("loss/mid", rets, grads, want32, want64, preds)
    rets2, grads2 = _run_loss(head, preds, {k: got[k] for k in TARGET_KEYS}, sliced=True)
    assert torch.equal(rets["loss"][0], rets2["loss"][0]) and all(torch.equal(grads[0][h], grads2[0][h]) for h in preds[0])


# ------------------------------------------------------------------------------------------------- end to end
def test_a_small_head_end_to_end(gold):
    """CenterHead in train(): forward (the composite route), loss, backward. Every parameter's gradient against the stock
    formulation through the same forward: float64 the truth, float32 the yardstick"""
    torch.manual_seed(0)
    head = _head("c10").train()
    x = _dev(T.synth.normal(T.SEED, "center/e2e/x", (2, 16, T.H, T.W)).astype(np.float32))
    ex = _example(recorded_targets(gold, "main"))
    cw, weight = T.CODES["c10"][1], T.CODES["c10"][2]

    def stock(h, x, dtype):
        preds = h(x)
        total = sum(T.task_loss(p, ex["hm"][t].to(dtype), ex["anno_box"][t].to(dtype), ex["ind"][t], ex["mask"][t], ex["cat"][t], cw, weight)[0]
                    for t, p in enumerate(preds))
        total.backward()
        return {k: _np(p.grad) for k, p in h.named_parameters()}, float(total.detach())

    truth, total64 = stock(copy.deepcopy(head).double(), x.double(), torch.float64)
    yard, _ = stock(copy.deepcopy(head), x, torch.float32)
    preds = head(x)
    rets = head.loss(ex, preds)
    total = sum(rets["loss"])
    total.backward()
    assert abs(float(total.detach()) - total64) <= 1e-5 * abs(total64)
    # the bias of a convolution that feeds a train-mode BatchNorm has a zero gradient by construction (the batch mean
    # removes it): what any run reports there is its own rounding noise, which is held to be small and not compared
    noise = {id(conv.bias) for seq in head._sequences() for conv, bn, _ in rpn._split(seq) if bn is not None}
    scale = max(np.abs(v).max() for v in truth.values())
    for k, p in head.named_parameters():
        assert p.grad is not None, k
        n = p.shape[0]
        if id(p) in noise:
            assert np.abs(truth[k]).max() <= 1e-12 * scale and float(p.grad.abs().max()) <= 1e-5 * scale, k
            continue
        _hold(f"e2e/grads/{k}", "param_grad", _np(p.grad).reshape(n, -1).T, yard[k].reshape(n, -1).T, truth[k].reshape(n, -1).T, structural_zeros=False)
