"""The second stage's training on the GPU (3dal_pytorch_amd/two_stage.py; dal3_roi_targets, dal3_roi_loss): the target
assignment against the reference's own record (tests/golden/roi_train.npz: discrete outputs exactly, copied outputs bit for
bit, floating outputs in multiples of the reference's fp32 error against its .double() run, roi_train_ref.BARS), the fused
form against the direct form and the sampled feature rows against `refine`'s bit for bit, the head step (losses, gradients,
running statistics), the status bit of a sample without fg and bg, `roi_loss` without a synchronisation, and
`second_stage_loss` end to end on tests/test_gpu_two_stage.py's detector. DAL3_ROI_TRAIN_RECORD=<path> writes every figure
held (how profiles/roi_train_measured.json is made)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import roi_ref as R
import roi_train_ref as T
import test_gpu_roi as Q
import test_gpu_two_stage as E
import test_gpu_voxelnet as V
from _common import golden
from roi_gpu import _dev, _rows
from test_gpu_two_stage import model  # noqa: F401

hip = importlib.import_module("3dal_pytorch_amd._hip")
pillars = importlib.import_module("3dal_pytorch_amd.pillars")
two_stage = importlib.import_module("3dal_pytorch_amd.two_stage")
pytestmark = pytest.mark.gpu

_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    path = os.environ.get("DAL3_ROI_TRAIN_RECORD")
    if path and _RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _grad_enabled():
    """the steps here build graphs, whatever an earlier test left switched"""
    with torch.enable_grad():
        yield


def _hold(row, kind, got, f32, truth):
    """each measure <= BARS[kind] x the reference's own fp32 error against its .double() run"""
    ratio, m, y = R.ratios(_rows(got), _rows(f32), _rows(truth))
    _RECORD[row] = {"kind": kind, "measured": {k: m[k] for k in R.MEASURES}, "yardstick": {k: y[k] for k in R.MEASURES}, "ratio": ratio}
    for k in R.MEASURES:
        print(f"{row:52s} {k:9s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:9.2f}  bar {T.BARS[kind]:g}")
    bad = [(k, m[k], ratio[k]) for k in R.MEASURES if not ratio[k] <= T.BARS[kind]]
    assert not bad, (row, bad)


def _want(g, tag, name):
    f32 = g[f"{tag}_{name}_f32"]
    return f32, f32.astype(np.float64) + g[f"{tag}_{name}_diff"].astype(np.float64)


def _inputs(tag):
    return T.big_inputs() if tag == "big" else T.golden_inputs(int(tag[1]))


def _targets(inp, cfg, **kw):
    return two_stage.roi_targets(cfg, inp["rois"].shape[-1], _dev(inp["gt_boxes_and_cls"]), _dev(inp["draws"]), rois=_dev(inp["rois"]),
                                 roi_scores=_dev(inp["roi_scores"]), roi_labels=_dev(inp["roi_labels"]), **kw)


@pytest.fixture(scope="module")
def gold():
    return golden("roi_train")


# ------------------------------------------------------------------------------------- the target assignment
@pytest.mark.parametrize("tag", ["c7", "c9", "big"])
def test_targets_equal_the_reference_record(gold, tag):
    inp = _inputs(tag)
    cfg = dict(T.TARGET, ROI_PER_IMAGE=T.BIG["R"]) if tag == "big" else T.TARGET
    t = _targets(inp, cfg)
    assert int(t["status"].item()) == 0
    got = {k: v.cpu().numpy() for k, v in t.items()}
    # discrete outputs: exactly
    assert np.array_equal(got["slot"], gold[f"{tag}_slot"]) and got["slot"].dtype == np.int32
    assert np.array_equal(got["sample"], gold[f"{tag}_sample"])
    assert np.array_equal(got["roi_labels"], gold[f"{tag}_roi_labels"]) and got["roi_labels"].dtype == np.int64
    assert np.array_equal(got["reg_valid_mask"], gold[f"{tag}_reg_valid_mask"])
    # copied outputs: bit for bit (gt_of_rois_src shows the assignment: the GT rows differ from one another)
    for name in ("rois", "roi_scores", "gt_of_rois_src"):
        assert np.array_equal(got[name], gold[f"{tag}_{name}_f32"]), name
    order = [0, 1, 2, 3, 4, 5, 7, 8, 6] if got["rois"].shape[-1] == 9 else list(range(7))
    assert np.array_equal(got["boxes"], got["rois"][..., order])               # the rotation back in the last column
    # floating outputs (the (B, R) ones as one column: their columns are no channels)
    for name in T.FLOAT_KEYS:
        f32, truth = _want(gold, tag, name)
        one = (lambda a: a.reshape(-1, 1)) if f32.ndim == 2 else (lambda a: a)
        _hold(f"targets/{tag}/{name}", name, one(got[name]), one(f32), one(truth))
    # the other CLS_SCORE_TYPE: -1 in the ignored band, from the same overlaps
    c = _targets(inp, dict(cfg, CLS_SCORE_TYPE="cls"))
    iou = gold[f"{tag}_gt_iou_of_rois_f32"]
    want = np.where((iou > 0.25) & (iou < 0.75), -1, (iou > 0.75).astype(np.int64))
    assert c["rcnn_cls_labels"].dtype == torch.int64 and np.array_equal(c["rcnn_cls_labels"].cpu().numpy(), want)
    assert (want == -1).any() and (want == 1).any() and (want == 0).any()
    assert torch.equal(c["slot"], t["slot"])


def test_a_sample_without_fg_and_bg_sets_the_status_bit_and_disturbs_nothing_else():
    inp = T.golden_inputs(7)
    clean = _targets(inp, T.TARGET)
    bad = {k: v.copy() for k, v in inp.items()}
    bad["rois"][1] = np.nan                       # every overlap of sample 1 is NaN: neither fg nor bg
    t = _targets(bad, T.TARGET)
    assert int(t["status"].item()) == hip.ROI_NO_SAMPLE == 8192
    for k in ("slot", "sample", "rois", "roi_labels", "roi_scores", "gt_iou_of_rois", "gt_of_rois_src", "reg_valid_mask",
              "rcnn_cls_labels", "gt_of_rois", "boxes"):
        assert torch.equal(t[k][0], clean[k][0]), k
        assert not t[k][1].to(torch.float32).clamp(min=0).any() and not torch.isnan(t[k][1].float()).any(), k
    assert (t["sample"][1] == -1).all()


# ------------------------------------------------------------------------------------- the head step
def _head(code, case):
    head = two_stage.RoIHead(R.NUM_POINT * R.MAP["C"], case["cfg"], code_size=code)
    head.load_state_dict({k: torch.as_tensor(v) for k, v in case["sd"].items()}, strict=True)
    return head.cuda().train()


def _all_features(case, inp):
    """roi_features (B, M, 100) of every slot by the eval modules: zero rows for the empty slots"""
    ext = two_stage.BEVFeatureExtractor(**R.EXTRACTOR)
    code = inp["rois"].shape[-1]
    feats = torch.zeros((2, T.M, 100), dtype=torch.float32).cuda()
    for b in range(2):
        live = np.nonzero(inp["roi_labels"][b])[0]
        box = inp["rois"][b][live]
        box = box[:, [0, 1, 2, 3, 4, 5, 7, 8, 6]] if code == 9 else box
        f = ext({"bev_feature": _dev(case["bev"][b:b + 1])}, [two_stage.box_points(_dev(box), 5)], 5)[0]
        feats[b, torch.as_tensor(live).cuda()] = f
    return feats


@pytest.mark.parametrize("code", [7, 9])
def test_head_step_equals_the_reference_record(gold, code):
    tag, case = f"c{code}", T.golden_case(code)
    inp = case["inp"]
    head = _head(code, case)
    batch = dict(rois=_dev(inp["rois"]), roi_scores=_dev(inp["roi_scores"]), roi_labels=_dev(inp["roi_labels"]),
                 gt_boxes_and_cls=_dev(inp["gt_boxes_and_cls"]), roi_features=_all_features(case, inp))
    out = head.train_forward(batch, _dev(inp["draws"]), drop_masks=[_dev(m) for m in case["masks"]])
    ret = head.forward_ret_dict
    assert out is batch and tuple(out["rois"].shape) == (2, T.ROWS, code) and out["batch_size"] == 2
    assert {"rois", "gt_of_rois", "gt_of_rois_src", "gt_iou_of_rois", "roi_scores", "roi_labels", "roi_features", "reg_valid_mask",
            "rcnn_cls_labels", "rcnn_cls", "rcnn_reg"} <= set(ret)
    f32, truth = _want(gold, tag, "features")
    _hold(f"step/{tag}/features", "head", ret["roi_features"].cpu().numpy(), f32, truth)
    ret["rcnn_cls"].retain_grad()
    ret["rcnn_reg"].retain_grad()
    loss, tb = head.get_loss()
    assert set(tb) == {"rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss"} and all(torch.is_tensor(v) and v.is_cuda for v in tb.values())
    loss.backward()
    for name, got in (("rcnn_cls", ret["rcnn_cls"]), ("rcnn_reg", ret["rcnn_reg"]), ("d_cls", ret["rcnn_cls"].grad),
                      ("d_reg", ret["rcnn_reg"].grad)):
        f32, truth = _want(gold, tag, name)
        _hold(f"step/{tag}/{name}", "grad" if name.startswith("d_") else "head", got.detach().cpu().numpy().reshape(f32.shape), f32, truth)
    f32, truth = _want(gold, tag, "loss")
    got = torch.stack([tb["rcnn_loss_cls"], tb["rcnn_loss_reg"], loss.detach()]).cpu().numpy()
    _hold(f"step/{tag}/loss", "loss", got[None], f32[None], truth[None])
    for k, p in head.named_parameters():
        f32, truth = _want(gold, tag, f"grads.{k}")
        assert p.grad is not None, k
        _hold(f"step/{tag}/grads/{k}", "grad", p.grad.cpu().numpy().reshape(f32.shape[0], -1), f32.reshape(f32.shape[0], -1),
              truth.reshape(f32.shape[0], -1))
    for k, v in head.state_dict().items():
        if "running" in k:
            f32, truth = _want(gold, tag, f"stats.{k}")
            _hold(f"step/{tag}/stats/{k}", "stats", v.cpu().numpy()[None], f32[None], truth[None])
        if "num_batches" in k:
            assert int(v) == 8
    # the layer losses one by one are the same launch's numbers
    assert torch.equal(head.get_box_cls_layer_loss(ret)[0], tb["rcnn_loss_cls"]) and torch.equal(head.get_box_reg_layer_loss(ret)[0], tb["rcnn_loss_reg"])


def _step_against_the_restatement(row, cfg, rows_per_sample, tag):
    """a head step on golden case c9's RoIs with `rows_per_sample` rows a sample and seeded (B, rows, 96) features, against
    roi_train_ref's float64 evaluation of the same step, the float32 one the yardstick"""
    code, c_in = 9, 96
    target = dict(T.TARGET, ROI_PER_IMAGE=rows_per_sample)
    cfg = dict(cfg, TARGET_CONFIG=target)
    inp = dict(T.golden_inputs(code), draws=R.synth.uniform(R.SEED, f"{tag}/draws", (2, T.M + rows_per_sample)).astype(np.float32))
    sd = R.head_weights(c_in, cfg, code, tag)
    feats = np.maximum(R.synth.uniform(R.SEED, f"{tag}/f", (2, rows_per_sample, c_in), -0.5, 2.0), 0.0).astype(np.float32)
    masks = T.drop_masks(cfg, 2 * rows_per_sample, tag)
    want = {}
    for dt in (T.F64, T.F32):
        tg = T.targets(inp, target, dt)
        params, stats = T.head_params(sd, dt)
        with torch.enable_grad():
            cls, reg = T.train_mlp(params, stats, cfg, T._t(feats, dt).view(-1, c_in), masks)
            loss = T.losses(cls, reg, tg, cfg["LOSS_CONFIG"])
            loss[2].backward()
        want[dt] = dict(slot=tg["slot"], loss=torch.stack(loss).detach(), grads={k: v.grad for k, v in params.items()}, stats=stats)
    head = two_stage.RoIHead(c_in, cfg, code_size=code)
    head.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    head = head.cuda().train()
    t = _targets(inp, target)
    assert torch.equal(t["slot"].cpu().long(), want[T.F64]["slot"])
    head._train_head(_dev(feats), t, [_dev(m) for m in masks])
    loss, tb = head.get_loss()
    loss.backward()
    got = torch.stack([tb["rcnn_loss_cls"], tb["rcnn_loss_reg"], loss.detach()]).cpu().numpy()
    _hold(f"{row}/loss", "loss", got[None], want[T.F32]["loss"].numpy()[None], want[T.F64]["loss"].numpy()[None])
    for k, p in head.named_parameters():
        n = p.shape[0]
        _hold(f"{row}/grads/{k}", "grad", p.grad.cpu().numpy().reshape(n, -1), want[T.F32]["grads"][k].numpy().reshape(n, -1),
              want[T.F64]["grads"][k].numpy().reshape(n, -1))
    for k, v in head.state_dict().items():
        if "running" in k:
            _hold(f"{row}/stats/{k}", "stats", v.cpu().numpy()[None], want[T.F32]["stats"][k].numpy()[None], want[T.F64]["stats"][k].numpy()[None])
    return head


def test_head_step_beyond_the_row_kernels_limit():
    """2 x 160 = 320 rows, more than dal3_tr_fc_max_rows(): every piece of the stacks takes train._FcTail"""
    assert 320 > hip.lib().dal3_tr_fc_max_rows()
    _step_against_the_restatement("tail320", R.model_cfg([64, 32], [32, 64], [32, 64]), 160, "tail320")


def test_head_step_with_one_width_branches():
    """CLS_FC / REG_FC of one width: the piece behind the Dropout holds the final convolution alone"""
    head = _step_against_the_restatement("onewidth", R.model_cfg([32], [48], [16]), 16, "onewidth")
    assert [len(s) for s in head._segments()] == [1, 2, 2] and head._segments()[1][1][0] == []


def test_l1_gradient_is_zero_at_zero_and_ignored_rows_carry_none():
    n, code = 300, 9                              # more rows than the workgroup's threads
    reg = torch.zeros((n, code)).cuda()
    tgt = torch.zeros((n, code + 1)).cuda()
    tgt[1::2, :code] = 1.0
    cls = torch.linspace(-9, 9, n).cuda().reshape(n, 1).requires_grad_(True)
    reg.requires_grad_(True)
    labels = torch.full((n,), 0.5).cuda()
    labels[::3] = -1.0
    valid = torch.ones(n, dtype=torch.int32).cuda()
    valid[:4] = 0
    loss = two_stage._RoILoss.apply(cls, reg, labels, valid, tgt, [1.0] * 7 + [0.2, 0.2], 1.0, 1.0)
    loss[2].backward()
    assert not reg.grad[0::2].any() and not reg.grad[:4].any()
    want = -torch.tensor([1.0] * 7 + [0.2, 0.2]).cuda() / (n - 4)
    assert torch.allclose(reg.grad[5], want, rtol=1e-6) and not cls.grad[::3].any() and cls.grad[1::3].abs().min() > 0
    p = torch.sigmoid(cls.detach().double().reshape(-1))
    keep = labels >= 0
    each = -(0.5 * torch.log(p) + 0.5 * torch.log(1 - p))[keep]
    assert abs(float(loss[0]) - float(each.mean())) < 1e-5 * float(each.mean())
    assert abs(float(loss[1]) - float((n // 2 - 2) * 7.4 / (n - 4))) < 1e-5 and float(loss[2]) == float(loss[0] + loss[1])


# ------------------------------------------------------------------------------------- the fused route, end to end
def _example():
    pts, off = V.sweep()
    r = pillars.voxelize(_dev(pts), off, V.VOXEL, V.RANGE, 5, 4000)
    voxels, coords, num, nv = r.finish()
    return dict(voxels=voxels, coordinates=coords, num_points=num, num_voxels=nv, shape=[V.GRID] * 2, metadata=V.META)


def _first_stage(m, example):
    with torch.no_grad():
        bev, _ = m.single_det.extract_feat(dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"],
                                                batch_size=2, input_shape=V.GRID))
        return bev, m.post().decode_nms(m.bbox_head(bev))


def _gt_from(r, out, n=6):
    """gt_boxes_and_cls (B, 8, 10) out of the first stage's own boxes: the first n of each sample, 5 % larger (an overlap of
    0.86 whatever the size: fg), two trailing zero rows. This detector keeps 0 and 2 boxes: sample 0 has no GT and only
    empty slots, sample 1 two fg RoIs and 81 empty slots."""
    B = out["boxes"].shape[0]
    rois = out_rois(r, out)
    gt = torch.zeros((B, n + 2, 10), dtype=torch.float32).cuda()
    for b in range(B):
        k = min(n, int(out["counts"][b]))
        gt[b, :k, :7] = rois[b, :k]
        gt[b, :k, 3:6] *= 1.05
        gt[b, :k, 9] = (out["labels"][b, :k] + 1).float()
    return gt


def test_fused_form_and_sampled_features_equal_the_direct_form_and_refine(model):
    m, _ = model
    m.eval()
    bev, r = _first_stage(m, _example())
    out = m.refine(r, bev)
    counts = out["counts"].tolist()
    assert max(counts) >= 2 and max(counts) < E.M
    gt = _gt_from(r, out)[:, :, [0, 1, 2, 3, 4, 5, 6, 9]].contiguous()
    cfg = dict(R.TARGET_CONFIG, ROI_PER_IMAGE=32)
    draws = _dev(R.synth.uniform(R.SEED, "e2e/draws", (2, E.M + 32)).astype(np.float32))
    live = torch.arange(E.M).cuda()[None, :] < out["counts"][:, None]
    direct = two_stage.roi_targets(cfg, 7, gt, draws, rois=out_rois(r, out), roi_scores=first_scores(r, out),
                                   roi_labels=torch.where(live, out["labels"] + 1, 0))
    r["status"].zero_()
    fused = two_stage.roi_targets(cfg, 7, gt, draws, fused=(r, [0]), M=E.M)
    assert int(fused["status"].item()) == 0 and set(fused) == set(direct)
    for k in direct:
        assert torch.equal(fused[k], direct[k]), k
    assert (fused["sample"] == -1).any() and (fused["sample"] >= 0).any() and fused["reg_valid_mask"].sum() > 0
    assert (fused["gt_iou_of_rois"] > 0.75).any()
    # the sampled rows of roi_loss are refine's rows of those slots, and zero for the empty slots
    m.roi_head.train()
    head_cfg = m.roi_head.target_config
    m.roi_head.target_config = cfg
    try:
        res = m.roi_loss(r, bev, gt, draws)
    finally:
        m.roi_head.target_config = head_cfg
        m.load_state_dict(model[1], strict=True)                               # the running statistics the step moved
        m.eval()
    t = res["targets"]
    assert torch.equal(t["slot"], fused["slot"])
    want = torch.gather(out["features"], 1, t["slot"].long().unsqueeze(-1).expand(-1, -1, out["features"].shape[-1]))
    want = want * (t["sample"] >= 0).unsqueeze(-1)
    # (this detector's 2 x 2 map gives zero rows for every box, as it does in refine: the rows of a map that does not are
    # held by test_sampled_feature_rows_are_refines_rows)
    assert torch.equal(t["roi_features"], want) and not t["roi_features"][t["sample"] < 0].any()


@pytest.mark.parametrize("code", [7, 9])
def test_sampled_feature_rows_are_refines_rows(code):
    """roi_loss on tests/test_gpu_roi.py's hand-built first-stage result (2 tasks, 3 samples: none, exactly M and M - 1 kept
    rows) over the 6 x 9 map: the ROI_PER_IMAGE gathered rows are refine's rows of the sampled slots bit for bit, zero
    for the empty slots, and every parameter of the head receives a gradient that is not zero"""
    M, rows = 11, 16
    case = R.golden_case(code)
    m = Q._detector(Q._head(100, case["cfg"], code, case["sd"]), M, Q.NUM_CLASSES)
    bev = _dev(R.bev_map("fused", B=Q.B)).permute(0, 3, 1, 2).contiguous()
    r = Q._first_stage_result(code, [[0, 4, 5], [0, 7, 5]])
    out = m.refine(r, bev)
    assert out["counts"].tolist() == [0, 11, 10] and int(out["status"].item()) == 0
    gt = torch.zeros((Q.B, 5, code + 1), dtype=torch.float32).cuda()
    for b, first in enumerate(Q._first_list(r, M)):
        k = min(3, first["scores"].numel())
        box = first["box3d_lidar"][:k]
        gt[b, :k, :code] = box[:, [0, 1, 2, 3, 4, 5, 8, 6, 7]] if code == 9 else box
        gt[b, :k, 3:6] *= 1.05
        gt[b, :k, code] = (first["label_preds"][:k] + 1).float()
    head = m.roi_head.train()
    head.target_config = dict(R.TARGET_CONFIG, ROI_PER_IMAGE=rows)
    draws = _dev(R.synth.uniform(R.SEED, f"rows/draws{code}", (Q.B, M + rows)).astype(np.float32))
    m.roi_loss(r, bev, gt, draws)                                              # warm
    head.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                    # both code sizes: nothing waits for the stream
    try:
        res = m.roi_loss(r, bev, gt, draws)
        res["loss"].backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    t = res["targets"]
    assert int(res["status"].item()) == 0 and tuple(t["roi_features"].shape) == (Q.B, rows, 100)
    want = torch.gather(out["features"], 1, t["slot"].long().unsqueeze(-1).expand(-1, -1, 100)) * (t["sample"] >= 0).unsqueeze(-1)
    assert torch.equal(t["roi_features"], want)
    assert (t["sample"][0] == -1).all() and (t["sample"][1] == 1).all() and (t["sample"][2] == 2).any()
    live = t["roi_features"][t["sample"] >= 0].abs().sum(-1) > 0              # a box with all five points off the map has a zero row
    assert not t["roi_features"][t["sample"] < 0].any() and int(live.sum()) >= 8
    # the sampled rois are the slots' rois, the labels the tasks' with their class offset, + 1
    box = torch.gather(out["labels"], 1, t["slot"].long())
    assert torch.equal(t["roi_labels"], torch.where(t["sample"] >= 0, box.long() + 1, 0))
    assert int(t["reg_valid_mask"][1].sum()) >= 3 and int(t["reg_valid_mask"][0].sum()) == 0
    for k, p in head.named_parameters():
        assert p.grad is not None and bool(p.grad.abs().sum() > 0), k


def out_rois(r, out):
    """refine's first-stage boxes per slot are not among its outputs (it refines them): the slots' rois through the modules'
    route, reorder_first_stage_pred_and_feature's layout (code 7: the box as it is)"""
    B, M = out["counts"].shape[0], E.M
    rois = torch.zeros((B, M, 7), dtype=torch.float32).cuda()
    for b in range(B):
        n = int(out["counts"][b])
        rows = r["keep"][b, :n].long() + int(r["seg_offsets"][b])
        rois[b, :n] = r["boxes"][rows]
    return rois


def first_scores(r, out):
    B, M = out["counts"].shape[0], E.M
    s = torch.zeros((B, M), dtype=torch.float32).cuda()
    for b in range(B):
        n = int(out["counts"][b])
        s[b, :n] = r["scores"][r["keep"][b, :n].long() + int(r["seg_offsets"][b])]
    return s


def test_second_stage_loss_trains_the_roi_head_alone_without_a_synchronisation(model):
    m, sd = model
    example = _example()
    m.eval()
    bev, r = _first_stage(m, example)
    example["gt_boxes_and_cls"] = _gt_from(r, m.refine(r, bev))
    with pytest.raises(RuntimeError, match="roi_head.train"):
        m.second_stage_loss(example)
    m.roi_head.train()
    draws = _dev(R.synth.uniform(R.SEED, "e2e/draws2", (2, E.M + 128)).astype(np.float32))
    try:
        # the device part may not synchronise (decode_nms uploads its segment offsets: it stays outside)
        gt = example["gt_boxes_and_cls"][:, :, [0, 1, 2, 3, 4, 5, 6, -1]].contiguous()
        m.roi_loss(r, bev, gt, draws)                                          # warm
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            res = m.roi_loss(r, bev, gt, draws)
            res["loss"].backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert int(res["status"].item()) == 0
        m.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        out = m.second_stage_loss(example, draws)
        assert list(out) == ["loss", "roi_reg_loss", "roi_cls_loss"] and all(len(v) == 1 for v in out.values())
        out["loss"][0].backward()
        with_grad = {k for k, p in m.named_parameters() if p.grad is not None}
        assert with_grad == {k for k, _ in m.named_parameters() if k.startswith("roi_head.")} and with_grad
        # (the 2 x 2 map's feature rows are zero, so the first layer's weight gradient is: the layers behind it learn)
        assert all(bool(p.grad.abs().sum() > 0) for k, p in m.roi_head.named_parameters() if k.endswith("bias"))
        # 20 Adam steps on one fixed batch with fixed draws lower the loss
        opt = torch.optim.Adam(m.roi_head.parameters(), lr=5e-3)
        losses = []
        for _ in range(21):
            opt.zero_grad(set_to_none=True)
            loss = m.second_stage_loss(example, draws)["loss"][0]
            losses.append(loss.detach())
            loss.backward()
            opt.step()
        losses = torch.stack(losses).cpu().numpy()
        print("loss over 20 Adam steps:", np.round(losses, 4).tolist())
        assert np.isfinite(losses).all() and losses[-1] < losses[0]
        with pytest.raises(NotImplementedError, match="freeze"):
            two_stage.TwoStageDetector(m.single_det, [m.second_stage[0]], m.roi_head, E.M, num_point=5, test_cfg=V.TEST_CFG).second_stage_loss(example)
    finally:
        m.load_state_dict(sd, strict=True)
        m.eval()
