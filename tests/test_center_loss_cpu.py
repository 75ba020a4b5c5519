"""The first stage's targets and loss without a GPU: tests/center_ref.py's restatement against the reference's own record
(tests/golden/center_loss.npz, written by tests/golden/gen_center_loss.py), the cases the inputs cover, the entries'
declarations, their argument errors and the refusals of CenterHead.loss and center_loss.center_targets."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import center_ref as T
from _common import ROOT, golden

hip = importlib.import_module("3dal_pytorch_amd._hip")
rpn = importlib.import_module("3dal_pytorch_amd.rpn")
center_loss = importlib.import_module("3dal_pytorch_amd.center_loss")

ENTRIES = ("dal3_center_targets", "dal3_center_loss", "dal3_center_loss_workspace_bytes")
TARGET_KEYS = ("hm", "anno_box", "ind", "mask", "cat")


def recorded_targets(g, tag):
    out = {k: [g[f"{tag}_t{t}_{k}"] for t in range(2)] for k in ("hm", "ind", "mask", "cat")}
    out["anno_box"] = [g[f"{tag}_t{t}_anno_box_f32"] for t in range(2)]
    out["anno_box64"] = [out["anno_box"][t].astype(np.float64) + g[f"{tag}_t{t}_anno_box_diff"].astype(np.float64) for t in range(2)]
    return out


@pytest.fixture(scope="module")
def gold():
    return golden("center_loss")


@pytest.mark.parametrize("tag", ["main", "empty"])
def test_target_restatement_equals_the_reference(gold, tag):
    want = recorded_targets(gold, tag)
    mine = T.targets(T.golden_gt(tag), T.NUM_CLASSES, T.VOXELS, 8, (T.H, T.W))
    for t in range(2):
        for k in TARGET_KEYS:
            assert mine[k][t].dtype == want[k][t].dtype and np.array_equal(mine[k][t], want[k][t]), (t, k)
        assert np.abs(mine["anno_box64"][t] - want["anno_box64"][t]).max() <= 1e-12
    assert [want[k][0].dtype for k in TARGET_KEYS] == [np.float32, np.float32, np.int64, np.uint8, np.int64]


@pytest.mark.parametrize("tag", ["main", "empty"])
@pytest.mark.parametrize("code", ["c10", "c8"])
def test_loss_restatement_equals_the_reference(gold, tag, code):
    _, cw, weight, with_vel = T.CODES[code]
    tg = recorded_targets(gold, tag)
    preds = T.head_maps(f"{tag}/{code}", tg, T.NUM_CLASSES, with_vel)
    m32, m64 = T.loss(preds, tg, cw, weight, T.F32), T.loss(preds, tg, cw, weight, T.F64)
    for t in range(2):
        assert len(m64[t]) == 5 + (6 if with_vel else 5)
        for name in m64[t]:
            f32 = gold[f"{tag}_{code}_t{t}_{name}_f32"]
            want = f32.astype(np.float64) + gold[f"{tag}_{code}_t{t}_{name}_diff"].astype(np.float64)
            assert np.abs(m64[t][name] - want).max() <= 1e-10 * max(np.abs(want).max(), 1e-30), (t, name)
            assert np.array_equal(m32[t][name], f32), (t, name)


def test_golden_inputs_cover_the_cases(gold):
    gt, tg = T.golden_gt("main"), recorded_targets(gold, "main")
    wc, lc, fx, fy = T.cells(gt, T.VOXELS, 8)
    m0, m1 = tg["mask"][0], tg["mask"][1]
    # slots are indexed by k: the skipped rows (w = 0, out of range, NaN, 1e20) leave zero rows between live ones
    assert m0[0].tolist()[:8] == [1, 1, 1, 0, 0, 1, 0, 0] and m0[1].tolist()[:5] == [1, 1, 0, 0, 0]
    assert not tg["anno_box"][0][0, 3].any() and wc[0, 3] == 0 and np.isnan(fx[0, 6]) and fy[0, 7] > 2.0 ** 31
    assert fx[0, 4] < -1 and fx[1, 2] >= T.W and fy[1, 3] < -1 and fy[1, 4] >= T.H
    # the centre in (-1, 0): kept at cell 0 with a negative offset
    assert -0.9 < fx[0, 5] < -0.1 and tg["ind"][0][0, 5] % T.W == 0 and tg["anno_box"][0][0, 5, 0] == fx[0, 5]
    # a padding gap: the second task's first row is row 9, its slot 0
    assert not gt[0, 8].any() and gt[0, 9, 9] == 2 and m1[0].tolist()[:7] == [1] * 6 + [0]
    # the four borders, a radius beyond the map (every pixel of its class lit), min_radius
    hm0, hm1 = tg["hm"][0], tg["hm"][1]
    assert hm0[0, 0, 10, 0] == 1 and hm0[0, 0, 9, 23] == 1 and hm1[0, 0, 0, 12] == 1 and hm1[0, 0, 19, 8] == 1
    assert (hm1[0, 0] > 0).all() and (hm0[0, 0, 2:7, 1:6] > 0).all() and int((hm0[0, 0, 0:9, 0:8] > 0).sum()) >= 25
    assert hm0[0, 0, 4, 3] == 1 and hm0[0, 0, 4, 6] == 0
    # two objects in one cell: the same class (task 0, sample 1), two classes (task 1, sample 1)
    assert tg["ind"][0][1, 0] == tg["ind"][0][1, 1] and tg["cat"][0][1, 0] == tg["cat"][0][1, 1]
    assert tg["ind"][1][1, 0] == tg["ind"][1][1, 2] and tg["cat"][1][1, 0] != tg["cat"][1][1, 2]
    # the empty task
    e = recorded_targets(gold, "empty")
    assert not e["mask"][1].any() and not e["hm"][1].any() and e["mask"][0].sum() == 6
    # both clamps bind, at an object's own pixel too, and one prediction equals its target
    p = T.head_maps("main/c10", tg, T.NUM_CLASSES, True)[0]
    s = 1 / (1 + np.exp(-p["hm"].astype(np.float64)))
    assert (s > 1 - 1e-4).sum() >= 3 and (s < 1e-4).sum() >= 3
    assert s[0, 0].reshape(-1)[tg["ind"][0][0, 0]] > 1 - 1e-4
    assert p["height"][1, 0].reshape(-1)[tg["ind"][0][1, 1]] == tg["anno_box"][0][1, 1, 2]
    g = gold["main_c10_t0_grad.hm_f32"]
    assert (g[(s > 1 - 1e-4) | (s < 1e-4)] == 0).all() and (g != 0).sum() > 900
    assert gold["empty_c10_t1_num_positive_f32"] == 0 and gold["empty_c10_t1_hm_loss_f32"] > 0 and gold["empty_c10_t1_loc_loss_f32"] == 0


def test_mid_inputs_fill_the_map():
    gt = T.mid_gt()
    m = T.MID
    tg = T.targets(gt, m["num_classes"], m["voxels"], m["out_size_factor"], (m["H"], m["W"]), max_objs=m["max_objs"])
    assert tg["mask"][0].sum() == 2 * m["objects"] and set(np.unique(tg["cat"][0])) == {0, 1, 2}
    assert (np.diff(gt[0, :, 9]) >= 0).all()


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dal3.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRIES:
        assert name + "(" in header and name in hip.SIGNATURES and hasattr(lib, name), name
    assert "DAL3_CENTER_OVERFLOW = 16384" in header and hip.CENTER_OVERFLOW == 16384
    for macro, v in (("OBJS", hip.CENTER_MAX_OBJS), ("CLASSES", hip.CENTER_MAX_CLASSES), ("COLS", hip.CENTER_MAX_COLS)):
        assert f"#define DAL3_CENTER_MAX_{macro} {v}" in header
    assert "dal3_center_loss.hip" in open(os.path.join(ROOT, "3dal_pytorch_amd", "csrc", "Makefile")).read()
    for struct, cls in (("dal3_center_targets_args", hip.CenterTargetsArgs), ("dal3_center_loss_args", hip.CenterLossArgs)):
        assert "} " + struct + ";" in header and cls.__doc__ == struct
    for name in ("center_targets", "AssignLabel", "FastFocalLoss", "RegLoss", "head_loss"):
        assert hasattr(center_loss, name)
    assert callable(rpn.CenterHead.loss) and callable(rpn.CenterHead.loss_from_gt)


def test_argument_errors():
    lib = hip.lib()
    assert lib.dal3_center_targets(None, None) == hip.EINVAL and lib.dal3_center_loss(None, None) == hip.EINVAL
    ok = dict(B=1, G=4, H=20, W=24, T=1, max_objs=16, out_size_factor=8.0, gaussian_overlap=0.1, min_radius=2)

    def targets(**kw):
        a = hip.CenterTargetsArgs(**dict(ok, **kw))
        a.voxel_size[0] = a.voxel_size[1] = kw.get("vs", 0.1)
        a.num_class[0] = kw.get("classes", 3)
        return a
    for bad, word in ((dict(B=-1), b"bad B"), (dict(G=0), b"bad B"), (dict(H=0), b"bad B"), (dict(W=70000), b"bad B"), (dict(T=0), b"T 0"),
                      (dict(T=17), b"T 17"), (dict(max_objs=0), b"max_objs 0"), (dict(max_objs=1025), b"max_objs 1025"),
                      (dict(vs=0.0), b"voxel_size"), (dict(out_size_factor=0.0), b"out_size_factor"),
                      (dict(gaussian_overlap=1.0), b"gaussian_overlap"), (dict(min_radius=-1), b"min_radius"),
                      (dict(classes=0), b"0 classes"), (dict(classes=65), b"65 classes"), (dict(), b"null output of task 0")):
        assert lib.dal3_center_targets(targets(**bad), None) == hip.EINVAL and word in lib.dal3_last_error(), (bad, lib.dal3_last_error())
    ok = dict(B=1, H=20, W=24, C=3, n_cols=10, max_objs=16)
    for bad, word in ((dict(B=-1), b"bad B"), (dict(C=0), b"bad B"), (dict(C=65), b"bad B"), (dict(n_cols=9), b"n_cols 9"),
                      (dict(max_objs=1025), b"max_objs 1025"), (dict(B=65535, H=65535, W=65535), b"2^31"), (dict(), b"vel map"),
                      (dict(n_cols=8), b"null out")):
        assert lib.dal3_center_loss(hip.CenterLossArgs(**dict(ok, **bad)), None) == hip.EINVAL and word in lib.dal3_last_error(), bad
    assert lib.dal3_center_loss_workspace_bytes(4, 3, 468, 468) >= 8 * (4 * 3 * 468 * 468 // 2048 + 4 * 11)
    assert lib.dal3_center_loss_workspace_bytes(4, 0, 468, 468) == 0 and lib.dal3_center_loss_workspace_bytes(-1, 3, 468, 468) == 0


def _head(**kw):
    args = dict(in_channels=16, tasks=T.TASKS, dataset="nuscenes", weight=0.25, code_weights=T.CODES["c10"][1], common_heads=T.HEADS9,
                share_conv_channel=64)
    return rpn.CenterHead(**dict(args, **kw))


def test_refusals():
    maps = lambda heads: [{h: torch.zeros(1, c, 4, 4) for h, c in dict(hm=1, **heads).items()}]       # noqa: E731
    nine = {h: T.CHANNELS[h] for h in T.REG_HEADS}
    seven = {h: c for h, c in nine.items() if h != "vel"}
    with pytest.raises(NotImplementedError, match="dataset 'kitti'"):
        _head(dataset="kitti", tasks=T.TASKS[:1]).loss({}, maps(nine))
    with pytest.raises(ValueError, match="code_weights is empty"):
        _head(code_weights=[], tasks=T.TASKS[:1]).loss({}, maps(nine))
    with pytest.raises(NotImplementedError, match="iou"):
        _head(tasks=T.TASKS[:1]).loss({}, maps(dict(nine, iou=1)))
    with pytest.raises(NotImplementedError, match="heads"):
        _head(tasks=T.TASKS[:1]).loss({}, maps({h: c for h, c in nine.items() if h != "rot"}))
    with pytest.raises(ValueError, match="10 entries"):
        _head(tasks=T.TASKS[:1]).loss({}, maps(seven))
    with pytest.raises(ValueError, match="1 prediction dictionaries for 2 tasks"):
        _head().loss({}, maps(nine))
    # the targets and the maps must be on the GPU: no CPU route, and it says so
    ex = {k: [torch.zeros(1)] for k in TARGET_KEYS}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _head(tasks=T.TASKS[:1]).loss(ex, maps(nine))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        center_loss.center_targets(torch.zeros(1, 4, 10), [1], T.VOXELS["range"], T.VOXELS["size"], 8, (20, 24))
    with pytest.raises(ValueError, match="AssignLabel needs"):
        center_loss.AssignLabel(cfg=T.ASSIGNER)(torch.zeros(1, 4, 10))
    a = center_loss.AssignLabel(cfg=T.ASSIGNER, voxels=T.VOXELS)
    assert a.num_classes == [1, 2] and a.out_size_factor == 8 and a._max_objs == 16 and a._min_radius == 2 and a.gaussian_overlap == 0.1
