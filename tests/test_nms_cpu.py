"""CPU-side checks of the detector post-processing (3dal_pytorch_amd/nms.py, detect.py; dal3_nms / dal3_center_decode):
the NumPy restatement of tests/nms_ref.py against what the reference's own rotate_nms_pcdet, circle_nms and
CenterHead.predict recorded (tests/golden/nms.npz, written by tests/golden/gen_nms.py), the C ABI's entries and argument
checks, and the refusals that need no device. No GPU compute here."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import nms_ref
from _common import ROOT, golden

hip = importlib.import_module("3dal_pytorch_amd._hip")
nms = importlib.import_module("3dal_pytorch_amd.nms")
detect = importlib.import_module("3dal_pytorch_amd.detect")

ENTRIES = ("dal3_nms_workspace_bytes", "dal3_nms", "dal3_center_decode_workspace_bytes", "dal3_center_decode")
HEAD_RUNS = {"ref_vel": ("ref", True), "ref_novel": ("ref", False), "small_vel": ("small", True), "circle_vel": ("circle", True)}


def scene():
    g = golden("nms")
    boxes, scores = nms_ref.clustered_scene(int(g["scene_seed"]))
    s = float(boxes.astype(np.float64).sum() + scores.astype(np.float64).sum())
    assert abs(s - float(g["scene_sum"])) < 1e-9, "the seeded scene drifted from the fixture"
    return g, boxes, scores


@pytest.mark.parametrize("case", sorted(nms_ref.SCENE_CASES))
def test_restated_nms_reproduces_the_references_kept_rows(case):
    g, boxes, scores = scene()
    mode, thresh, pre, post = nms_ref.SCENE_CASES[case]
    want = g[f"scene_{case}_keep"]
    assert 0 < want.size < boxes.shape[0]
    assert np.array_equal(nms_ref.nms(boxes, scores, mode, thresh, pre, post, mirror=True), want)


def test_the_scene_exercises_the_sequential_dependence_and_the_conversion():
    """greedy keeps more than 'no higher box overlaps' would, and without rotate_nms_pcdet's conversion of the boxes the
    kept rows differ: it is not an isometry of the pair"""
    g, boxes, scores = scene()
    o = nms_ref.order(scores)
    sup = np.triu(nms_ref.suppression(nms_ref.mirrored(boxes[o]), "rotate", 0.7), 1)
    assert nms_ref.greedy(sup).size > int((~sup.any(0)).sum())
    assert not np.array_equal(nms_ref.nms(boxes, scores, "rotate", 0.7, 4096, 500, mirror=False), g["scene_rotate_ref_keep"])


def test_stable_order_nan_first_ties_by_row():
    s = np.array([0.5, np.nan, 0.5, 0.9, -0.0, 0.0, np.nan, -np.inf, np.inf], np.float32)
    assert nms_ref.order(s).tolist() == [1, 6, 8, 3, 0, 2, 4, 5, 7]


@pytest.mark.parametrize("run", sorted(HEAD_RUNS))
def test_restated_decode_and_predict_reproduce_the_reference(run):
    g = golden("nms")
    cfg_name, vel = HEAD_RUNS[run]
    cfg = nms_ref.CONFIGS[cfg_name]
    tasks = nms_ref.head_maps(int(g["head_seed"]), vel)
    for t, task in enumerate(tasks):
        for b, (cell, label, boxes, score) in enumerate(nms_ref.decode(task, cfg)):
            key = f"head_{run}_t{t}_b{b}_"
            assert np.array_equal(cell, g[key + "cell"]) and np.array_equal(label, g[key + "label"])
            want = g[key + "boxes"]
            exact = [0, 1, 2] + ([6, 7] if vel else [])
            assert np.array_equal(boxes[:, exact].view(np.uint32), want[:, exact].view(np.uint32))
            np.testing.assert_allclose(boxes, want, rtol=1e-5, atol=0)
            np.testing.assert_allclose(score, g[key + "score"], rtol=1e-5, atol=0)
    for b, ret in enumerate(nms_ref.predict(tasks, cfg)):
        want = g[f"head_{run}_ret{b}_boxes"]
        assert ret[0].shape == want.shape and want.shape[0] > 0
        np.testing.assert_allclose(ret[0], want, rtol=1e-5, atol=0)
        assert np.array_equal(ret[2], g[f"head_{run}_ret{b}_labels"])


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dal3.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRIES:
        assert name + "(" in header and name in hip.SIGNATURES and hasattr(lib, name), name
    assert "#define DAL3_NMS_MAX_PRE 65536" in header and hip.NMS_MAX_PRE == 65536
    assert hip.lib().dal3_version() == 170
    assert "dal3_nms.hip" in open(os.path.join(ROOT, "3dal_pytorch_amd", "csrc", "Makefile")).read()
    # O(K): twice the rows, twice the bytes (to the 256-byte sections)
    one, two = hip.lib().dal3_nms_workspace_bytes(1 << 16, 0), hip.lib().dal3_nms_workspace_bytes(1 << 17, 0)
    assert two == 2 * one and hip.lib().dal3_nms_workspace_bytes(1 << 16, 1) > one


FAKE = 0x1000                                   # never dereferenced: every case fails before a launch


def _nms_args(off=(0, 4, 4, 10), **kw):
    off = np.asarray(off, np.int64)
    a = hip.NmsArgs(F=off.size - 1, K=10, seg_offsets=FAKE, seg_offsets_host=off.ctypes.data, boxes=FAKE, scores=FAKE,
                    box_stride=7, yaw_col=6, mode=hip.NMS_ROTATE, thresh=0.7, stride=6, keep=FAKE, keep_count=FAKE,
                    status=FAKE, workspace=FAKE, workspace_bytes=1 << 20)
    for k, v in kw.items():
        setattr(a, k, v)
    return a, off


def test_nms_argument_errors_without_a_gpu():
    lib = hip.lib()
    assert lib.dal3_nms(None, None) == hip.EINVAL and b"null args" in lib.dal3_last_error()
    for kw, what in ((dict(keep=None), b"null keep"), (dict(keep_count=None), b"null keep_count"),
                     (dict(status=None), b"null keep_count / status"), (dict(stride=5), b"stride 5 too small"),
                     (dict(pre_max=hip.NMS_MAX_PRE + 1), b"DAL3_NMS_MAX_PRE"), (dict(mode=2), b"unknown mode"),
                     (dict(seg_offsets_host=None), b"seg_offsets_host"), (dict(yaw_col=7), b"box layout"),
                     (dict(box_stride=6), b"box layout"), (dict(boxes_f64=2), b"boxes_f64"), (dict(mirror=2), b"mirror"),
                     (dict(post_max=-1), b"negative"), (dict(workspace=None), b"null boxes / scores / workspace")):
        a, off = _nms_args(**kw)
        assert lib.dal3_nms(a, None) == hip.EINVAL, kw
        assert what in lib.dal3_last_error(), (kw, lib.dal3_last_error())
    for off in ((0, 5, 3, 10), (0, 4, 11), (-1, 4, 10)):
        a, keepalive = _nms_args(off=off)
        assert lib.dal3_nms(a, None) == hip.EINVAL and b"non-decreasing" in lib.dal3_last_error(), off
    a, off = _nms_args(post_max=3, stride=3)            # post_max bounds the stride
    a.workspace_bytes = 16
    assert lib.dal3_nms(a, None) == hip.EWORKSPACE
    a, off = _nms_args(off=(0,))                        # no segment: nothing to do, nothing dereferenced
    assert lib.dal3_nms(a, None) == 0
    assert lib.dal3_nms_workspace_bytes(-1, 0) == 0 and lib.dal3_nms_workspace_bytes(8, 2) == 0


def test_decode_argument_errors_without_a_gpu():
    lib = hip.lib()
    assert lib.dal3_center_decode(None, None) == hip.EINVAL

    def args(**kw):
        m = hip.Map(FAKE, 1, 1, 1, 1)
        a = hip.CenterDecodeArgs(B=2, H=4, W=4, C=1, hm=m, reg=m, height=m, dim=m, rot=m, F=2, K=32, seg_first=0, seg_step=1,
                                 seg_offsets=FAKE, boxes=FAKE, scores=FAKE, labels=FAKE, cell=FAKE, seg_count=FAKE, status=FAKE,
                                 workspace=FAKE, workspace_bytes=1 << 20)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw in (dict(C=0), dict(C=65), dict(H=0), dict(seg_first=1), dict(seg_step=0), dict(F=1), dict(hm=hip.Map()),
               dict(boxes=None), dict(seg_count=None), dict(status=None), dict(workspace=None), dict(H=1 << 13, W=1 << 13)):
        assert lib.dal3_center_decode(args(**kw), None) == hip.EINVAL, kw
    assert lib.dal3_center_decode(args(workspace_bytes=0), None) == hip.EWORKSPACE
    assert lib.dal3_center_decode(args(B=0), None) == 0


def test_python_refusals_without_a_gpu():
    cfg = nms_ref.as_test_cfg(nms_ref.CONFIGS["ref"])
    for key in ("double_flip", "per_class_nms"):
        with pytest.raises(ValueError, match=key):
            detect.CenterHeadPost(dict(cfg, **{key: True}), [1, 2])
    detect.CenterHeadPost(cfg, [1, 2])
    cpu = torch.zeros((4, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nms.rotate_nms_pcdet(cpu, torch.zeros(4), 0.7)
    with pytest.raises(TypeError):
        nms.batched_nms(np.zeros((4, 7)), torch.zeros(4), [0, 4], "rotate", 0.7)
    with pytest.raises(ValueError, match="mode"):
        nms.batched_nms(cpu, torch.zeros(4), [0, 4], "soft", 0.7)
    with pytest.raises(ValueError, match="token"):
        detect.CenterHeadPost.to_prediction([{"box3d_lidar": cpu, "scores": cpu, "label_preds": cpu, "metadata": None}])
