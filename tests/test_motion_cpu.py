"""The motion-state run without a GPU: the NumPy restatement (tests/motion_ref.py) against what the reference's own
trackGT.py / motionState.py recorded (tests/golden/motion.npz), the host side of the file-level run (the flattening of
the track dicts), the SVM fit against scikit-learn's recorded model, and the C header's new entries."""
import importlib
import os
import re

import numpy as np
import pytest

import motion_ref
from _common import ROOT, golden

motion = importlib.import_module("3dal_pytorch_amd.motion")
hip = importlib.import_module("3dal_pytorch_amd._hip")

# float64 features against the recorded ones (the issue's bound): the operation order is NumPy's up to the final 3-term
# dot and sqrt; deviations of 1e-2 m taken at 1e4 m carry 2e-12 absolute each -> 1e-10 relative on the variance, x 10
RTOL = 1e-9


@pytest.fixture(scope="module")
def scenes():
    return {"train": motion_ref.scene(**motion_ref.TRAIN), "val": motion_ref.scene(**motion_ref.VAL)}


def test_restated_gt_table_equals_trackgt_py(scenes):
    g = golden("motion")
    for name in ("train", "val"):
        gt = motion_ref.gt_table(scenes[name][0])
        assert list(gt.keys()) == list(g[f"gt_{name}_names"])
        assert np.array_equal([o["static"] for o in gt.values()], g[f"gt_{name}_static"])
        assert np.array_equal([len(o["box"]) for o in gt.values()], g[f"gt_{name}_len"])
        assert np.array_equal(np.array([o["box"][0] for o in gt.values()]), g[f"gt_{name}_first_box"])
        assert 0 < g[f"gt_{name}_static"].sum() < len(gt)


def test_restated_features_equal_motionstate_py(scenes):
    g = golden("motion")
    for name in ("train", "val"):
        frames, tracks = scenes[name]
        gt = motion_ref.gt_table(frames)
        X, Y, ids = motion_ref.track_feature(tracks, gt)
        assert ids == list(g[f"{name}_keep_ids"])
        assert np.array_equal(Y, g[f"{name}Y"])
        np.testing.assert_allclose(X, g[f"{name}X"], rtol=RTOL, atol=0)
        # the flat form the kernels take gives the same table
        flat = motion.flatten_tracks(tracks, gt)
        start, entry = motion_ref.group(flat["keys"], len(tracks))
        f = motion_ref.features(start, entry, flat["center"], flat["type"], flat["score"], flat["n_points"], flat["match"])
        keep = f["keep"].astype(bool)
        assert [k for k, kept in zip(tracks, keep) if kept] == ids
        np.testing.assert_allclose(f["feature"][keep], g[f"{name}X"], rtol=RTOL, atol=0)
        static = np.array([o["static"] for o in gt.values()])
        assert np.array_equal(static[f["match_last"][keep]], g[f"{name}Y"])
    # what the scene is meant to hold is there
    n = np.array([len(o["bbox"]) for o in scenes["train"][1].values()])
    assert (n < 7).any() and (n >= 7).any()
    assert any(o["match"][-1] is None for o in scenes["train"][1].values())
    assert any(o["type"][0] == 2 for o in scenes["train"][1].values())
    assert any(sum(len(p) for p in o["point"]) == 0 for o in scenes["train"][1].values())
    assert np.abs(scenes["train"][1][next(iter(scenes["train"][1]))]["bbox"][0][:2]).max() > 1e3


def test_train_split_lists_are_the_reference_files(scenes):
    g = golden("motion")
    frames, tracks = scenes["train"]
    gt = motion_ref.gt_table(frames)
    _, Y, ids = motion_ref.track_feature(tracks, gt)
    for kind, label in (("trackStatic", 1), ("trackDynamic", 0)):
        lst = [i for i, y in zip(ids, Y) if y == label]
        assert lst == list(g[f"train_{kind}_ids"])
        counts = [len(lst) * (i + 1) // 16 - len(lst) * i // 16 for i in range(16)]
        assert counts == list(g[f"train_{kind}_counts"])


def test_group_restatement_is_the_stable_argsort():
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 50, 1000)
    start, entry = motion_ref.group(keys, 50)
    assert np.array_equal(entry, np.argsort(keys, kind="stable"))
    assert np.array_equal(np.diff(start), np.bincount(keys, minlength=50))


def test_fit_linear_svm_against_the_recorded_svc():
    """the yardstick is libsvm's own stop (tol = 1e-3): |d_ours - d_ref| <= 1e-3 (1 + |d_ref|) on every val row, the
    labels equal on every val row with |d_ref| > 2e-3; at most 1 % of the rows may lie inside that band"""
    g = golden("motion")
    info = {}
    w, b = motion.fit_linear_svm(g["trainX"], g["trainY"], info=info)
    assert info["violation"] < 1e-4                         # ten times tighter than libsvm's default
    d = g["valX"] @ w + b
    ref = g["decision"]
    err = np.abs(d - ref) / (1 + np.abs(ref))
    print(f"svm: max |d - d_ref| / (1 + |d_ref|) = {err.max():.3e}, iterations {info['iterations']}, {info['seconds']:.3f} s")
    assert (np.abs(ref) <= 2e-3).mean() <= 0.01
    assert err.max() <= 1e-3
    clear = np.abs(ref) > 2e-3
    assert np.array_equal((d > 0)[clear], g["y_pred"][clear] == 1)
    # the dual point is feasible
    a = info["alpha"]
    ys = np.where(g["trainY"] > 0, 1.0, -1.0)
    assert a.min() >= 0 and a.max() <= 1 and abs(float(a @ ys)) < 1e-9


def test_fit_linear_svm_refuses_one_class():
    with pytest.raises(ValueError):
        motion.fit_linear_svm(np.zeros((4, 2)), np.ones(4))


def test_model_file_round_trip(tmp_path):
    p = str(tmp_path / "motion_svm.json")
    motion.save_model(p, np.array([-2.5, 0.125]), 1.75)
    w, b = motion.load_model(p)
    assert list(w) == [-2.5, 0.125] and b == 1.75


def test_header_declares_the_motion_entries():
    text = open(os.path.join(ROOT, "include", "dal3.h")).read()
    assert int(re.search(r"^#define\s+DAL3_VERSION\s+(\d+)", text, re.M).group(1)) == hip.lib().dal3_version()
    for name in ("dal3_group_workspace_bytes", "dal3_group_by_key", "dal3_track_features", "dal3_gt_table",
                 "dal3_motion_classify_workspace_bytes", "dal3_motion_classify"):
        assert re.search(rf"\b{name}\(", text), name
        assert name in hip.SIGNATURES
        assert hasattr(hip.lib(), name)
    for name in ("dal3_group_args", "dal3_track_feature_args", "dal3_gt_table_args", "dal3_motion_classify_args"):
        assert name in text
    assert int(re.search(r"DAL3_MOTION_BAD_KEY = (\d+)", text).group(1)) == hip.MOTION_BAD_KEY
    assert hip.MOTION_BAD_KEY not in (hip.TRACK_OVERFLOW, hip.TRACK_BAD_LABEL, hip.TRACK_BAD_ID)
    # argument checks that need no device
    lib = hip.lib()
    assert lib.dal3_group_by_key(None, None) == hip.EINVAL
    assert lib.dal3_group_workspace_bytes(-1, 4) == 0 and lib.dal3_group_workspace_bytes(4096, 10) > 3 * 4096 * 4
