"""The second stage's training without a GPU: tests/roi_train_ref.py's restatement against the reference's own record
(tests/golden/roi_train.npz, written by tests/golden/gen_roi_train.py), the planted faults against the GPU tests' bars, the
entries' declarations, their argument errors and the refusals of 3dal_pytorch_amd/two_stage.py's training route."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import roi_ref as R
import roi_train_ref as T
from _common import ROOT, golden
from test_roi_cpu import MODEL, TEST_CFG

hip = importlib.import_module("3dal_pytorch_amd._hip")
two_stage = importlib.import_module("3dal_pytorch_amd.two_stage")

ENTRIES = ("dal3_roi_targets", "dal3_roi_loss")


def _rows(a):
    a = a.detach().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a[:, None]


@pytest.fixture(scope="module")
def runs():
    """the float64 truth and the float32 yardstick of both golden cases, computed once"""
    out = {}
    for code in (7, 9):
        c = T.golden_case(code)
        out[code] = (c, T.run(c["sd"], c["cfg"], c["bev"], c["inp"], c["masks"], T.F64), T.run(c["sd"], c["cfg"], c["bev"], c["inp"], c["masks"], T.F32))
    return out


def _flat(r):
    out = {k: r[k] for k in ("rois", "roi_scores", "gt_of_rois_src", "gt_iou_of_rois", "rcnn_cls_labels", "gt_of_rois", "features",
                             "rcnn_cls", "rcnn_reg", "loss", "d_cls", "d_reg") if k in r}
    for group in ("grads", "stats"):
        out.update({f"{group}.{k}": v for k, v in r.get(group, {}).items()})
    return {k: v.detach().numpy() for k, v in out.items()}


def _check(g, tag, truth, yard):
    t, y = _flat(truth), _flat(yard)
    for name in t:
        want = g[f"{tag}_{name}_f32"].astype(np.float64) + g[f"{tag}_{name}_diff"].astype(np.float64)
        assert t[name].shape == want.shape, name
        assert np.abs(t[name] - want).max() <= 1e-10 * max(np.abs(want).max(), 1e-30), name
    for name in ("rois", "roi_scores", "gt_of_rois_src", "gt_iou_of_rois", "rcnn_cls_labels", "gt_of_rois"):
        # the float32 restatement is the reference's own formulation: the same stock ops, the same bits
        assert np.array_equal(y[name], g[f"{tag}_{name}_f32"]), name
    for name in ("slot", "sample", "roi_labels", "reg_valid_mask"):
        assert np.array_equal(truth[name].numpy(), g[f"{tag}_{name}"]) and np.array_equal(yard[name].numpy(), g[f"{tag}_{name}"]), name


@pytest.mark.parametrize("code", [7, 9])
def test_restatement_equals_the_reference(runs, code):
    _check(golden("roi_train"), f"c{code}", runs[code][1], runs[code][2])


def test_restatement_equals_the_reference_at_the_production_sort_width():
    inp, cfg = T.big_inputs(), dict(T.TARGET, ROI_PER_IMAGE=T.BIG["R"])
    _check(golden("roi_train"), "big", T.targets(inp, cfg, T.F64), T.targets(inp, cfg, T.F32))


def test_golden_samples_cover_the_cases(runs):
    g = golden("roi_train")
    c7, c9 = runs[7][1], runs[9][1]
    iou7, iou9 = c7["gt_iou_of_rois"].numpy(), c9["gt_iou_of_rois"].numpy()
    # c7 sample 0: fg and bg, the permutation cut at ROWS / 2, fewer hard bg (3) than the cap (6), easy bg behind them
    assert (iou7[0, :8] >= 0.55).all() and ((iou7[0, 8:11] >= 0.1) & (iou7[0, 8:11] < 0.55)).all() and (iou7[0, 11:] < 0.1).all()
    assert int((T.golden_inputs(7)["roi_labels"][0] != 0).sum()) == 40
    # c7 sample 1: fg only, 48 slots, drawn with replacement
    assert (iou7[1] >= 0.55).all() and len(set(c7["slot"][1].tolist())) < T.ROWS
    # c9 sample 0: 5 fg, hard-only bg; sample 1: no GT, easy-only bg, empty slots among the rows
    assert (iou9[0, :5] >= 0.55).all() and ((iou9[0, 5:] >= 0.1) & (iou9[0, 5:] < 0.55)).all()
    assert not iou9[1].any() and not c9["gt_of_rois_src"][1].any() and (c9["sample"][1] == -1).any() and (c9["sample"][1] == 1).any()
    # a class without GT (label 3 beside GT of classes 1 and 2), interior and trailing zero GT rows
    inp = T.golden_inputs(7)
    gt0 = inp["gt_boxes_and_cls"][0]
    assert (inp["roi_labels"][0] == 3).any() and 3 not in gt0[:, -1] and not gt0[3].any() and not gt0[5].any() and gt0[8].any() and not gt0[9:].any()
    # headings on both sides of the flip: rois turned by pi against their GT, and not
    d = np.abs(c7["gt_of_rois_src"][..., 6].numpy() - T.limit_period(c7["rois"][..., 6], 0.5, 2 * np.pi).numpy()) % (2 * np.pi)
    fg = iou7 >= 0.55
    assert ((d[fg] > 3.0) & (d[fg] < 3.3)).any() and ((d[fg] < 0.1) | (d[fg] > 6.2)).any()
    assert T.stability(c7) >= 1e-3 and T.stability(c9) >= 1e-3
    assert g["big_slot"].shape == (1, 128) and len(set(g["big_slot"][0, :64].tolist())) == 64


def test_every_planted_fault_shows(runs):
    assert set(T.FAULTS) == {"fg_strict", "tie_highest", "flip_missing", "pick_unclamped"}
    case, truth, yard = runs[7]
    # a `>` for the `>=` at fg_thresh: an overlap of exactly the threshold is fg
    o = torch.tensor([0.9, 0.55, 0.3, 0.0], dtype=torch.float64)
    cfg = dict(T.TARGET, ROI_PER_IMAGE=4)
    key, pick = np.asarray([0.5, 0.1, 0.0, 0.0], np.float32), np.zeros(4, np.float32)
    assert T.subsample(o, cfg, key, pick).tolist() == [1, 0, 2, 3] and T.subsample(o, cfg, key, pick, "fg_strict").tolist() == [0, 2, 3, 3]
    # the highest index among equal maxima: a background RoI far from its class's GT rows is assigned the last of them
    bad = T.targets(case["inp"], case["cfg"]["TARGET_CONFIG"], T.F64, "tie_highest")
    assert torch.equal(bad["slot"], truth["slot"]) and not torch.equal(bad["gt_of_rois_src"], truth["gt_of_rois_src"])
    tie, _, _ = R.ratios(_rows(bad["gt_of_rois"]), _rows(yard["gt_of_rois"]), _rows(truth["gt_of_rois"]))
    print("tie_highest", tie)
    # the unclamped pick: a product that rounds up to n indexes past the list
    assert T.draw(np.float32(1.0), 7) == 6 and T.draw(np.float32(1.0), 7, "pick_unclamped") == 7
    assert T.draw(np.nextafter(np.float32(1), np.float32(0)), 43) == 42
    # the missing flip, in multiples of the yardstick
    bad = T.targets(case["inp"], case["cfg"]["TARGET_CONFIG"], T.F64, "flip_missing")
    ratio, _, _ = R.ratios(_rows(bad["gt_of_rois"]), _rows(yard["gt_of_rois"]), _rows(truth["gt_of_rois"]))
    print("flip_missing", ratio)
    # the two faults that show in a floating output (the other two move a slot or an index, which the GPU tests compare exactly)
    smallest = min(max(ratio.values()), max(tie.values()))
    assert smallest >= T.SMALLEST_FAULT_RATIO and smallest / T.BARS["gt_of_rois"] >= 10.0
    assert max(T.BARS.values()) <= T.SMALLEST_FAULT_RATIO / 10.0


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dal3.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRIES:
        assert name + "(" in header and name in hip.SIGNATURES and hasattr(lib, name), name
    assert "DAL3_ROI_NO_SAMPLE = 8192" in header and hip.ROI_NO_SAMPLE == 8192
    for macro, v in (("M", hip.ROI_TRAIN_MAX_M), ("R", hip.ROI_TRAIN_MAX_R), ("G", hip.ROI_TRAIN_MAX_G)):
        assert f"#define DAL3_ROI_TRAIN_MAX_{macro} {v}" in header
    assert "dal3_roi_train.hip" in open(os.path.join(ROOT, "3dal_pytorch_amd", "csrc", "Makefile")).read()
    assert "} dal3_roi_targets_args;" in header and hip.RoiTargetsArgs.__doc__ == "dal3_roi_targets_args"
    for name in ("ProposalTargetLayer", "roi_targets"):
        assert hasattr(two_stage, name)
    for name in ("assign_targets", "get_loss", "get_box_reg_layer_loss", "get_box_cls_layer_loss", "train_forward"):
        assert callable(getattr(two_stage.RoIHead, name))
    assert all(hasattr(two_stage.TwoStageDetector, n) for n in ("roi_loss", "second_stage_loss"))
    assert two_stage.RoIHead(100, R.SMALL, code_size=7).forward_ret_dict is None


def test_argument_errors():
    lib = hip.lib()
    ok = dict(B=1, M=48, R=16, G=12, code_size=7, cls_thresh_span=0.5, hard_bg_ratio=0.8, fg_per_image=8)
    for bad, word in ((dict(M=513), b"bad B / M"), (dict(M=0), b"bad B / M"), (dict(R=513), b"bad B / M"), (dict(R=0), b"bad B / M"),
                      (dict(G=1025), b"bad B / M"), (dict(G=0), b"bad B / M"), (dict(code_size=8), b"code_size"),
                      (dict(B=-1), b"bad B / M"), (dict(cls_score_type=2), b"cls_score_type"), (dict(hard_bg_ratio=1.5), b"hard_bg_ratio"),
                      (dict(cls_thresh_span=0.0), b"cls_thresh_span"), (dict(), b"direct form needs")):
        a = hip.RoiTargetsArgs(**dict(ok, **bad))
        assert lib.dal3_roi_targets(a, None) == hip.EINVAL and word in lib.dal3_last_error(), bad
    assert lib.dal3_roi_targets(None, None) == hip.EINVAL
    assert lib.dal3_roi_targets(hip.RoiTargetsArgs(**dict(ok, B=0)), None) == hip.OK          # no sample: nothing to do
    cw = (ctypes.c_float * 9)(*([1.0] * 9))
    assert lib.dal3_roi_loss(None, None, 4, 8, None, None, None, cw, 1.0, 1.0, None, None, None, None) == hip.EINVAL
    assert b"code_size" in lib.dal3_last_error()
    assert lib.dal3_roi_loss(None, None, 4, 9, None, None, None, cw, 1.0, 1.0, None, None, None, None) == hip.EINVAL
    assert b"null" in lib.dal3_last_error()


def test_refusals():
    m = two_stage.TwoStageDetector(**dict(MODEL, freeze=False), test_cfg=TEST_CFG)
    with pytest.raises(NotImplementedError, match="freeze"):
        m.second_stage_loss({})
    m = two_stage.TwoStageDetector(**MODEL, test_cfg=TEST_CFG).eval()
    with pytest.raises(RuntimeError, match="roi_head.train"):
        m.second_stage_loss({})
    with pytest.raises(RuntimeError, match="single_det.eval"):
        m.train().second_stage_loss({})
    with pytest.raises(NotImplementedError, match="training"):
        m.roi_head({}, training=True)
    ret = {"rcnn_cls": torch.zeros(2, 1), "rcnn_reg": torch.zeros(2, 9)}
    for bad, word in ((dict(CLS_LOSS="CrossEntropy"), "CrossEntropy"), (dict(REG_LOSS="smooth-l1"), "smooth-l1")):
        head = two_stage.RoIHead(2560, dict(R.PRODUCTION, LOSS_CONFIG=dict(R.LOSS_CONFIG, **bad)), code_size=9)
        with pytest.raises(NotImplementedError, match=word):
            head.get_box_cls_layer_loss(ret)
        head.forward_ret_dict = ret
        with pytest.raises(NotImplementedError, match=word):
            head.get_loss()
    with pytest.raises(RuntimeError, match="before train_forward"):
        two_stage.RoIHead(2560, R.PRODUCTION, code_size=9).get_loss()
    # limits, the class-agnostic assignment and an unknown score type, by name, before anything is launched
    gt = torch.zeros((1, 4, 10))
    for kw, word in ((dict(rois=torch.zeros((1, 600, 9))), "600 slots"), (dict(rois=torch.zeros((1, 48, 9)), cfg=dict(ROI_PER_IMAGE=600)), "ROI_PER_IMAGE = 600"),
                     (dict(rois=torch.zeros((1, 48, 9)), gt=torch.zeros((1, 1100, 10))), "1100 GT rows")):
        cfg = dict(R.TARGET_CONFIG, **kw.get("cfg", {}))
        with pytest.raises(ValueError, match=word):
            two_stage.roi_targets(cfg, 9, kw.get("gt", gt), None, rois=kw["rois"], roi_scores=torch.zeros(kw["rois"].shape[:2]),
                                  roi_labels=torch.zeros(kw["rois"].shape[:2], dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="SAMPLE_ROI_BY_EACH_CLASS"):
        two_stage.roi_targets(dict(R.TARGET_CONFIG, SAMPLE_ROI_BY_EACH_CLASS=False), 9, gt, None, rois=torch.zeros((1, 48, 9)))
    with pytest.raises(NotImplementedError, match="CLS_SCORE_TYPE"):
        two_stage.roi_targets(dict(R.TARGET_CONFIG, CLS_SCORE_TYPE="raw_roi_iou"), 9, gt, None, rois=torch.zeros((1, 48, 9)))
