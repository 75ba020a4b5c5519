"""CPU-side checks of the double-flip test-time augmentation (dal3_flip4_points, dal3_center_decode_flip4; detect.
DoubleFlipPost, pillars.double_flip): the NumPy restatement of tests/tta_ref.py against what the reference's own
CenterHead.predict with double_flip and its DoubleFlip recorded (tests/golden/tta.npz, written by tests/golden/gen_tta.py),
the C ABI's entries and argument checks, and the refusals that need no device. No GPU compute here."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import nms_ref
import tta_ref
from _common import ROOT, golden

hip = importlib.import_module("3dal_pytorch_amd._hip")
detect = importlib.import_module("3dal_pytorch_amd.detect")
pillars = importlib.import_module("3dal_pytorch_amd.pillars")

ENTRIES = ("dal3_center_decode_flip4_workspace_bytes", "dal3_center_decode_flip4", "dal3_flip4_points")
CELLS = tta_ref.HEAD["H"] * tta_ref.HEAD["W"]


@pytest.mark.parametrize("run", sorted(tta_ref.RUNS))
def test_restated_merge_and_predict_reproduce_the_reference(run):
    g = golden("tta")
    cfg_name, vel = tta_ref.RUNS[run]
    cfg = nms_ref.CONFIGS[cfg_name]
    tasks = tta_ref.head_maps(int(g["tta_seed"]), vel)
    exact = [0, 1, 2] + ([6, 7] if vel else [])
    for t, task in enumerate(tasks):
        merged = tta_ref.merge_decode(task, cfg)
        assert len(merged) == 2
        for b, (cell, label, boxes, score) in enumerate(merged):
            key = f"tta_{run}_t{t}_b{b}_"
            assert 0 < cell.size < CELLS
            assert np.array_equal(cell, g[key + "cell"]) and np.array_equal(label, g[key + "label"])
            want = g[key + "boxes"]
            assert np.array_equal(boxes[:, exact].view(np.uint32), want[:, exact].view(np.uint32))
            np.testing.assert_allclose(boxes, want, rtol=1e-5, atol=0)
            np.testing.assert_allclose(score, g[key + "score"], rtol=1e-5, atol=0)
    for b, ret in enumerate(tta_ref.predict(tasks, cfg)):
        want = g[f"tta_{run}_ret{b}_boxes"]
        assert ret[0].shape == want.shape and want.shape[0] > 0
        np.testing.assert_allclose(ret[0], want, rtol=1e-5, atol=0)
        assert np.array_equal(ret[2], g[f"tta_{run}_ret{b}_labels"])


def test_the_merge_is_not_the_decode_of_any_one_view():
    """the fixture's views are independent: a merge that dropped or repeated a view would not pass by accident"""
    g = golden("tta")
    cfg = nms_ref.CONFIGS["ref"]
    task = tta_ref.head_maps(int(g["tta_seed"]), True)[1]
    merged = tta_ref.merge_decode(task, cfg)
    for v in range(4):
        one = nms_ref.decode({k: m[v::4] for k, m in task.items()}, cfg)
        assert all(not np.array_equal(a[0], b[0]) for a, b in zip(one, merged))


def test_flip4_points_is_the_references_double_flip_bit_for_bit():
    g = golden("tta")
    pts = tta_ref.sweep()
    assert abs(float(pts.astype(np.float64).sum()) - float(g["flip_sum"])) < 1e-9, "the seeded sweep drifted from the fixture"
    out, off = tta_ref.flip4_points(pts, [0, pts.shape[0]])
    n = pts.shape[0]
    assert off.tolist() == [0, n, 2 * n, 3 * n, 4 * n]
    for v, want in enumerate((pts, g["flip_yflip"], g["flip_xflip"], g["flip_double"])):
        assert out[off[v]:off[v + 1]].view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), v
    assert np.signbit(g["flip_yflip"][3, 1]) and not np.signbit(g["flip_yflip"][4, 1])     # 0.0 -> -0.0 and back
    # several samples, one empty: each sample's four views are consecutive
    out, off = tta_ref.flip4_points(pts, [0, 10, 10, n])
    assert off.tolist() == [0, 10, 20, 30, 40, 40, 40, 40, 40, 40 + (n - 10), 40 + 2 * (n - 10), 40 + 3 * (n - 10), 4 * n]
    assert np.array_equal(out[off[9]:off[10], 1], -pts[10:, 1]) and np.array_equal(out[off[9]:off[10], 0], pts[10:, 0])
    assert np.array_equal(out[off[10]:off[11], 0], -pts[10:, 0]) and np.array_equal(out[off[2]:off[3], :2], pts[:10, :2] * [-1, 1])


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dal3.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRIES:
        assert name + "(" in header and name in hip.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct dal3_center_decode_flip4_args" in header
    assert hip.lib().dal3_version() == 170


def test_workspace_bytes_formula_at_two_sizes():
    """one int32 per (merged sample, chunk of 1024 cells), in the carver's 256-byte sections: dal3_center_decode's own"""
    lib = hip.lib()
    for B, H, W in ((2, 12, 20), (3, 468, 468)):
        chunks = (H * W + 1023) // 1024
        want = (4 * B * chunks + 255) // 256 * 256
        assert lib.dal3_center_decode_flip4_workspace_bytes(B, H, W) == want == lib.dal3_center_decode_workspace_bytes(B, H, W)
    assert lib.dal3_center_decode_flip4_workspace_bytes(-1, 4, 4) == 0
    assert lib.dal3_center_decode_flip4_workspace_bytes(1, 1 << 13, 1 << 13) == 0


FAKE = 0x1000                                   # never dereferenced: every case fails before a launch


def test_merge_decode_argument_errors_without_a_gpu():
    lib = hip.lib()
    assert lib.dal3_center_decode_flip4(None, None) == hip.EINVAL and b"null args" in lib.dal3_last_error()

    def args(**kw):
        m = hip.Map(FAKE, 1, 1, 1, 1)
        d = hip.CenterDecodeArgs(B=2, H=4, W=4, C=1, hm=m, reg=m, height=m, dim=m, rot=m, F=2, K=32, seg_first=0, seg_step=1,
                                 seg_offsets=FAKE, boxes=FAKE, scores=FAKE, labels=FAKE, cell=FAKE, seg_count=FAKE, status=FAKE,
                                 workspace=FAKE, workspace_bytes=1 << 20)
        for k, v in kw.items():
            setattr(d, k, v)
        return hip.CenterDecodeFlip4Args(decode=d)

    for kw in (dict(C=0), dict(C=65), dict(H=0), dict(W=0), dict(B=-1), dict(B=(1 << 22) + 1), dict(seg_first=1),
               dict(seg_step=0), dict(F=1), dict(hm=hip.Map()), dict(rot=hip.Map()), dict(boxes=None), dict(cell=None),
               dict(seg_offsets=None), dict(seg_count=None), dict(status=None), dict(workspace=None),
               dict(max_workgroups=-1), dict(H=1 << 13, W=1 << 13)):
        assert lib.dal3_center_decode_flip4(args(**kw), None) == hip.EINVAL, kw
        assert b"center_decode_flip4" in lib.dal3_last_error(), kw
    assert lib.dal3_center_decode_flip4(args(workspace_bytes=0), None) == hip.EWORKSPACE
    assert b"dal3_center_decode_flip4_workspace_bytes" in lib.dal3_last_error()
    assert lib.dal3_center_decode_flip4(args(B=0), None) == 0      # nothing to do, nothing dereferenced


def test_flip4_points_argument_errors_without_a_gpu():
    lib = hip.lib()

    def call(points=FAKE, N=8, C=5, offsets=FAKE, B=2, out=FAKE, out_offsets=FAKE, max_workgroups=0):
        return lib.dal3_flip4_points(points, N, C, offsets, B, out, out_offsets, max_workgroups, None)

    for kw in (dict(C=1), dict(C=65), dict(N=-1), dict(B=-1), dict(N=(1 << 22) + 1), dict(B=(1 << 22) + 1), dict(points=None),
               dict(out=None), dict(offsets=None), dict(out_offsets=None), dict(max_workgroups=-1)):
        assert call(**kw) == hip.EINVAL, kw
        assert b"flip4_points" in lib.dal3_last_error(), kw
    assert call(B=0) == 0 and call(B=0, N=0, points=None, out=None, offsets=None, out_offsets=None) == 0


def test_python_refusals_without_a_gpu():
    cfg = nms_ref.as_test_cfg(nms_ref.CONFIGS["ref"])
    flip = dict(cfg, double_flip=True)
    with pytest.raises(ValueError, match="double_flip"):           # the one-view class still refuses it
        detect.CenterHeadPost(flip, [1, 2])
    with pytest.raises(ValueError, match="per_class_nms"):
        detect.DoubleFlipPost(dict(flip, per_class_nms=True), [1, 2])
    post = detect.DoubleFlipPost(flip, [1, 2], capacity=7)
    assert post.VIEWS == 4 and post.capacity == 7 and isinstance(post, detect.CenterHeadPost)
    maps = [{k: torch.from_numpy(v) for k, v in t.items()} for t in tta_ref.head_maps(0)]
    for n in (1, 2, 3, 5, 7):                                      # refused, not asserted, and before anything is enqueued
        short = [{k: v[:n] for k, v in t.items()} for t in maps]
        with pytest.raises(ValueError, match="multiple"):
            post.decode(short)
        with pytest.raises(ValueError, match="multiple"):
            post.predict(short)
    for n in (1, 3, 4, 7, 9):                                      # 8 maps are two samples: 2 or 8 entries
        with pytest.raises(ValueError, match="metadata"):
            post.predict(maps, metadata=[{"token": str(i)} for i in range(n)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        post.decode(maps)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pillars.double_flip(torch.zeros((4, 5)), [0, 4])
    with pytest.raises(TypeError):
        pillars.double_flip(np.zeros((4, 5), np.float32), [0, 4])
