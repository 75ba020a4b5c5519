"""CenterPoint's second stage without a GPU: tests/roi_ref.py's restatements against the reference's own outputs
(tests/golden/roi.npz, written by tests/golden/gen_roi.py), the planted faults against the GPU tests' bars, the fold, and
the host side of 3dal_pytorch_amd/two_stage.py: construction from the two-stage config's dictionaries, checkpoint keys,
refusals, exports and the workspace size."""
import ctypes
import importlib
import math
import os

import numpy as np
import pytest
import torch

import roi_ref as R
from _common import ROOT, golden

hip = importlib.import_module("3dal_pytorch_amd._hip")
two_stage = importlib.import_module("3dal_pytorch_amd.two_stage")
detector = importlib.import_module("3dal_pytorch_amd.detector")

ENTRIES = ("dal3_bev_gather", "dal3_box_points", "dal3_roi_pack_floats", "dal3_roi_pack", "dal3_roi_head_workspace_bytes",
           "dal3_roi_head", "dal3_roi_post")
TASKS = [dict(num_class=3, class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"])]
FIRST = dict(type="VoxelNet", reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5),
             backbone=dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8),
             neck=dict(type="RPN", layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[32, 64], us_layer_strides=[1, 2],
                       us_num_filters=[64, 64], num_input_features=256),
             bbox_head=dict(type="CenterHead", in_channels=128, tasks=TASKS, dataset="waymo", weight=2, code_weights=[1.0] * 10,
                            common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}))
TEST_CFG = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0],
                nms=dict(nms_pre_max_size=1000, nms_post_max_size=83, nms_iou_threshold=0.2), score_threshold=0.02,
                pc_range=[-4.0, -4.0], out_size_factor=8, voxel_size=[0.5, 0.5])
MODEL = dict(first_stage_cfg=FIRST,
             second_stage_modules=[dict(type="BEVFeatureExtractor", pc_start=[-75.2, -75.2], voxel_size=[0.1, 0.1], out_stride=8)],
             roi_head=dict(type="RoIHead", input_channels=128 * 5, model_cfg=R.PRODUCTION, code_size=9),
             NMS_POST_MAXSIZE=500, num_point=5, freeze=True)


def _rows(a):
    a = np.asarray(a)
    return a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a[:, None]


def _flat(r):
    return {"centres": torch.cat(r["centres"]).numpy(), "features": torch.cat(r["features"]).numpy(), "cls": r["cls"].numpy(),
            "box_preds": r["box_preds"].numpy(), "final_boxes": torch.cat([f[0] for f in r["final"]]).numpy(),
            "final_scores": torch.cat([f[1] for f in r["final"]]).numpy()}


@pytest.fixture(scope="module")
def runs():
    """the float64 truth and the float32 yardstick of both golden cases, computed once"""
    out = {}
    for code in (7, 9):
        case = R.golden_case(code)
        out[code] = (case, R.second_stage(case["sd"], case["cfg"], code, case["bev"], case["pred"], dtype=R.F64),
                     R.second_stage(case["sd"], case["cfg"], code, case["bev"], case["pred"], dtype=R.F32))
    return out


@pytest.mark.parametrize("code", [7, 9])
def test_restatements_equal_the_reference(runs, code):
    g, tag = golden("roi"), f"c{code}"
    _, truth, yard = runs[code]
    t, y = _flat(truth), _flat(yard)
    for name in t:
        want = g[f"{tag}_{name}_f32"].astype(np.float64) + g[f"{tag}_{name}_diff"].astype(np.float64)
        assert t[name].shape == want.shape
        assert np.abs(t[name] - want).max() <= 1e-11 * np.abs(want).max(), name
        # the float32 restatement is the reference's own formulation: the same stock ops, the same bits
        assert np.array_equal(y[name], g[f"{tag}_{name}_f32"]), name
    labels = torch.cat([f[2] for f in truth["final"]]).numpy()
    assert labels.dtype == np.int64 and np.array_equal(labels, g[f"{tag}_final_labels"])
    assert [f[0].shape[0] for f in truth["final"]] == list(g[f"{tag}_final_counts"]) == list(R.GOLDEN_BOXES)


def test_production_head_equals_the_reference():
    g, case = golden("roi"), R.production_case()
    cls, box = R.head_alone(case)
    for name, mine in (("cls", cls), ("box_preds", box)):
        want = g[f"prod_{name}_f32"].astype(np.float64) + g[f"prod_{name}_diff"].astype(np.float64)
        assert np.abs(mine.numpy() - want).max() <= 1e-11 * np.abs(want).max(), name
        assert R.judge(_rows(g[f"prod_{name}_f32"]), _rows(want))["tensor"] < 1e-5


def test_golden_inputs_cover_the_map_and_its_outside(runs):
    case, truth, _ = runs[9]
    W, H = R.MAP["W"], R.MAP["H"]
    x, y = R.relative(torch.cat(truth["centres"]).numpy())
    assert (x < 0).any() and (x > W - 1).any() and (y < 0).any() and (y > H - 1).any()
    inside = (x > 0) & (x < W - 1) & (y > 0) & (y < H - 1)
    assert 0.3 < float(inside.double().mean()) < 0.9
    rot = np.concatenate([p["box3d_lidar"][:, -1] for p in case["pred"]])
    assert (rot > np.pi).any() and (rot < -np.pi).any()


# which output shows a fault, and in which golden case
FAULT_SHOWS = {"xy_swapped": (9, "features"), "hw_swapped": (9, "features"), "weights_unclamped": (9, "features"),
               "sections_interleaved": (9, "features"), "front_back_swapped": (9, "features"), "rot_column_6": (9, "features"),
               "eps_1e-3": (7, "box_preds"), "velocity_rotated": (9, "box_preds"), "sqrt_dropped": (7, "final_scores")}


def test_every_planted_fault_is_ten_bars_away(runs):
    assert set(FAULT_SHOWS) | {"labels_not_shifted"} == set(R.FAULTS)
    smallest = {}
    for fault, (code, name) in FAULT_SHOWS.items():
        case, truth, yard = runs[code]
        bad = R.second_stage(case["sd"], case["cfg"], code, case["bev"], case["pred"], dtype=R.F64, fault=fault)
        ratio, _, _ = R.ratios(_rows(_flat(bad)[name]), _rows(_flat(yard)[name]), _rows(_flat(truth)[name]))
        worst = max(ratio[k] / R.BARS[k] for k in R.MEASURES)
        smallest[fault] = max(ratio.values())
        print(f"{fault:22s} {name:13s} " + "  ".join(f"{k} {ratio[k]:.3g}" for k in R.MEASURES))
        assert worst >= 10.0, (fault, ratio)
    print("smallest fault ratio:", min(smallest.values()), min(smallest, key=smallest.get))
    assert R.SMALLEST_FAULT_RATIO is not None and min(smallest.values()) >= R.SMALLEST_FAULT_RATIO
    assert max(R.BARS.values()) <= R.SMALLEST_FAULT_RATIO / 10.0
    case, truth, _ = runs[7]
    bad = R.second_stage(case["sd"], case["cfg"], 7, case["bev"], case["pred"], fault="labels_not_shifted")
    assert all(not torch.equal(a[2], b[2]) and torch.equal(a[2] + 1, b[2]) for a, b in zip(truth["final"], bad["final"]))


def test_fold_is_a_float64_evaluation_rounded_once():
    case = R.golden_case(9)
    sd = case["sd"]
    for conv, bn, _ in R.layer_names(case["cfg"]):
        w, bias = sd[conv + "weight"], sd.get(conv + "bias")
        wf, bf = R.fold(w, bias, None if bn is None else R.bn_of(sd, bn), 1e-5)
        assert wf.dtype == np.float32 and bf.dtype == np.float32 and wf.shape == (w.shape[0], w.shape[1])
        for co in (0, w.shape[0] // 2, w.shape[0] - 1):
            if bn is None:
                assert wf[co, 1] == w[co, 1, 0] and bf[co] == bias[co]
                continue
            g, beta, mean, var = (float(v[co]) for v in R.bn_of(sd, bn))
            scale = g / math.sqrt(var + 1e-5)
            assert wf[co, 1] == np.float32(float(w[co, 1, 0]) * scale)
            assert bf[co] == np.float32((0.0 - mean) * scale + beta)


# ------------------------------------------------------------------------------------- the host side of two_stage.py
def test_the_three_classes_build_from_the_config_dictionaries():
    m = two_stage.TwoStageDetector(**MODEL, test_cfg=TEST_CFG, max_points=5, max_voxels=4000, voxel_size=(0.5, 0.5, 0.1),
                                   pc_range=(-4.0, -4.0, -2.0, 4.0, 4.0, 2.0))
    assert isinstance(m.single_det, detector.VoxelNet) and m.bbox_head is m.single_det.bbox_head
    assert isinstance(m.second_stage[0], two_stage.BEVFeatureExtractor) and m.second_stage[0].out_stride == 8
    assert isinstance(m.roi_head, two_stage.RoIHead) and m.roi_head.code_size == 9
    assert m.NMS_POST_MAXSIZE == 500 and m.num_point == 5 and m.single_det.test_cfg is TEST_CFG
    assert m.roi_head.target_config == R.TARGET_CONFIG and m.roi_head.loss_config == R.LOSS_CONFIG
    keys = set(m.state_dict())
    first = set(m.single_det.state_dict())
    assert keys == {"single_det." + k for k in first} | {"bbox_head." + k for k in m.bbox_head.state_dict()} | \
        {"roi_head." + k for k in m.roi_head.state_dict()}
    assert any(k.startswith("bbox_head.") for k in keys) and any(k.startswith("single_det.bbox_head.") for k in keys)
    # a checkpoint with the duplicated keys loads strictly
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()}, strict=True)
    pp = two_stage.TwoStageDetector(dict(type="PointPillars", reader=dict(type="PillarFeatureNet", num_filters=[64, 64], num_input_features=5,
                                         with_distance=False, voxel_size=(0.32, 0.32, 6.0), pc_range=(-5.12, -5.12, -2, 5.12, 5.12, 4.0)),
                                         backbone=dict(type="PointPillarsScatter", ds_factor=1), neck=FIRST["neck"] | dict(num_input_features=64),
                                         bbox_head=FIRST["bbox_head"]), MODEL["second_stage_modules"], MODEL["roi_head"], 100, num_point=5)
    assert isinstance(pp.single_det, detector.PointPillars)


def test_roi_head_keys_and_shapes_are_the_reference_list():
    g = golden("roi")
    head = two_stage.RoIHead(2560, R.PRODUCTION, code_size=9)
    sd = head.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]]
    for k, shape in zip(g["keys"], g["key_shapes"]):
        assert list(sd[str(k)].shape) == [int(d) for d in shape[:sd[str(k)].dim()]], k
    assert isinstance(head.shared_fc_layer[3], torch.nn.Dropout) and isinstance(head.cls_layers[3], torch.nn.Dropout)
    head.load_state_dict({k: torch.as_tensor(v) for k, v in R.production_case()["sd"].items()}, strict=True)
    small = two_stage.RoIHead(100, R.SMALL, code_size=7)
    assert set(small.state_dict()) == set(R.head_weights(100, R.SMALL, 7))
    s = small.shape()
    assert (s.c_in, s.n_shared, s.n_cls, s.n_reg, list(s.shared)[:2], list(s.cls)[:2], list(s.reg)[:2], s.code_size) == \
        (100, 2, 2, 2, [32, 32], [16, 48], [16, 48], 7)
    # an attribute object serves as model_cfg as well
    obj = type("Cfg", (), R.SMALL)
    assert list(two_stage.RoIHead(100, obj, code_size=7).state_dict()) == list(small.state_dict())


def test_refusals():
    m = two_stage.TwoStageDetector(**MODEL, test_cfg=TEST_CFG)
    with pytest.raises(NotImplementedError, match="loss is not built"):
        m.eval()({}, return_loss=True)
    with pytest.raises(NotImplementedError, match="training"):
        m.roi_head({}, training=True)
    with pytest.raises(ValueError, match="double_flip"):
        two_stage.TwoStageDetector(**MODEL, test_cfg=dict(TEST_CFG, double_flip=True))
    with pytest.raises(KeyError, match="first stage type 'SECOND'"):
        two_stage.TwoStageDetector(dict(FIRST, type="SECOND"), MODEL["second_stage_modules"], MODEL["roi_head"], 500)
    for bad in (dict(SHARED_FC=[250, 256]), dict(CLS_FC=[512]), dict(REG_FC=[16, 16, 16, 16]), dict(SHARED_FC=[])):
        with pytest.raises(ValueError, match="serves 1 to 3 widths"):
            two_stage.RoIHead(2560, dict(R.PRODUCTION, **bad), code_size=9)
    with pytest.raises(ValueError, match="num_class"):
        two_stage.RoIHead(2560, R.PRODUCTION, num_class=3)
    with pytest.raises(ValueError, match="code_size"):
        two_stage.RoIHead(2560, R.PRODUCTION, code_size=8)
    with pytest.raises(NotImplementedError, match="second stage.*TwoStageDetector"):
        m.single_det.forward_two_stage({})


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dal3.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRIES:
        assert name + "(" in header and name in hip.SIGNATURES and hasattr(lib, name), name
    assert "DAL3_ROI_OVERFLOW = 4096" in header and hip.ROI_OVERFLOW == 4096
    assert f"#define DAL3_ROI_MAX_WIDTH {hip.ROI_MAX_WIDTH}" in header and f"#define DAL3_ROI_MAX_TASKS {hip.ROI_MAX_TASKS}" in header
    assert "dal3_roi.hip" in open(os.path.join(ROOT, "3dal_pytorch_amd", "csrc", "Makefile")).read()
    for name in ("BEVFeatureExtractor", "RoIHead", "TwoStageDetector", "box_points"):
        assert hasattr(two_stage, name)
    for struct in (hip.BevGatherArgs, hip.RoiShape, hip.RoiHeadArgs):
        assert struct.__doc__.strip() + " {" in header or "} " + struct.__doc__.strip() + ";" in header


def test_workspace_bytes_and_pack_floats():
    lib = hip.lib()
    ws = lib.dal3_roi_head_workspace_bytes
    sizes = [[ws(B, M, 5, 512, 9) for M in (1, 11, 500, 2000)] for B in (1, 2, 4)]
    assert all(s > 0 for row in sizes for s in row)
    assert all(a < b for row in sizes for a, b in zip(row, row[1:]))                      # monotone in M
    assert all(a < b for col in zip(*sizes) for a, b in zip(col, col[1:]))                # and in B
    assert ws(4, 500, 5, 512, 9) >= 4 * 500 * 2560 * 4
    assert ws(0, 0, 5, 512, 9) == ws(0, 500, 1, 1, 7) == 0                                # no sample: nothing to hold
    for bad in ((-1, 500, 5, 512, 9), (1, -5, 5, 512, 9), (1, 500, 3, 512, 9), (1, 500, 5, 0, 9), (1, 500, 5, 512, 8),
                (70000, 1, 5, 512, 9), (4096, 8192, 5, 512, 9)):
        assert ws(*bad) == 0, bad
    head = two_stage.RoIHead(2560, R.PRODUCTION, code_size=9)
    want = sum(-(-co // 32) * 32 + -(-co // 32) * -(-ci // 8) * 256
               for ci, co in [(2560, 256), (256, 256), (256, 256), (256, 256), (256, 1), (256, 256), (256, 256), (256, 9)])
    assert lib.dal3_roi_pack_floats(head.shape()) == want
    s = head.shape()
    s.shared[0] = 250
    assert lib.dal3_roi_pack_floats(s) == 0
    a = hip.RoiHeadArgs(shape=s)
    assert lib.dal3_roi_head(a, None) == hip.EINVAL and b"not served" in lib.dal3_last_error()
    g = hip.BevGatherArgs(B=1, H=6, W=9, C=20, n=4, points_per_row=7)
    assert lib.dal3_bev_gather(g, None) == hip.EINVAL and b"points_per_row" in lib.dal3_last_error()
    assert lib.dal3_box_points(None, 4, 8, 5, None, None) == hip.EINVAL
    assert lib.dal3_roi_post(None, None, None, 4, 8, None, None, None) == hip.EINVAL
