"""The motion-state command lines (python -m 3dal_pytorch_amd.motion gt / --track_train --track_val) on the seeded train
and val work dirs of tests/motion_ref.py, against what the reference's tools/trackGT.py and tools/motionState.py wrote
and printed on the same dirs (tests/golden/motion.npz)."""
import importlib
import os
import pickle

import numpy as np
import pytest

import motion_ref
from _common import golden

motion = importlib.import_module("3dal_pytorch_amd.motion")
pytestmark = pytest.mark.gpu
RTOL = 1e-9


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _same_track(a, b):
    assert list(a.keys()) == list(b.keys()) == ["type", "bbox", "score", "point", "match", "token"]
    assert a["type"] == b["type"] and a["match"] == b["match"] and a["token"] == b["token"] and a["score"] == b["score"]
    assert all(np.array_equal(x, y) for x, y in zip(a["bbox"], b["bbox"])) and len(a["bbox"]) == len(b["bbox"])
    assert all(np.array_equal(x, y) for x, y in zip(a["point"], b["point"])) and len(a["point"]) == len(b["point"])


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("motion"))
    train, val, tr, va = motion_ref.write_work_dirs(root)
    for wd in (train, val):
        motion.main(["gt", "--infos", os.path.join(wd, "infos.pkl"), "--result", os.path.join(wd, "trackGT.pkl")])
    return {"train": (train, tr), "val": (val, va)}


def test_gt_command_writes_the_reference_trackgt(dirs):
    g = golden("motion")
    for name in ("train", "val"):
        wd, (frames, _) = dirs[name]
        gt = _load(os.path.join(wd, "trackGT.pkl"))
        assert list(gt.keys()) == list(g[f"gt_{name}_names"])
        assert [o["static"] for o in gt.values()] == list(g[f"gt_{name}_static"])         # exact
        want = motion_ref.gt_table(frames)
        for key, obj in gt.items():
            ref = want[key]
            assert list(obj.keys()) == ["box", "vel", "pose", "num_points", "static"]
            assert obj["num_points"] == ref["num_points"] and type(obj["static"]) is int
            assert np.array_equal(obj["pose"], ref["pose"]) and obj["pose"].shape == (4, 4)
            assert all(b.shape == (7,) and b.dtype == np.float64 for b in obj["box"])
            np.testing.assert_allclose(np.array(obj["box"]), np.array(ref["box"]), rtol=RTOL, atol=1e-12)
            assert all(v.dtype == np.float32 for v in obj["vel"])                         # the dtype of obj['box'], as np.linalg.norm gives
            np.testing.assert_allclose(np.array(obj["vel"]), np.array(ref["vel"]), rtol=4e-7, atol=0)   # float32: the dot, the sqrt and our one rounding, <= 3 ulp
        np.testing.assert_allclose(np.array([o["box"][0] for o in gt.values()]), g[f"gt_{name}_first_box"], rtol=RTOL, atol=1e-12)


def test_motion_command_writes_the_reference_files_and_lines(dirs, capsys):
    g = golden("motion")
    (train, (_, tr_tracks)), (val, (_, va_tracks)) = dirs["train"], dirs["val"]
    capsys.readouterr()
    motion.main(["--track_train", train, "--track_val", val])
    out = capsys.readouterr().out
    assert f"Number of train: {int(g['n_train'])}" in out and f"Number of val: {int(g['n_val'])}" in out
    # train: split by the GT flag — exact
    for kind in ("trackStatic", "trackDynamic"):
        parts = [_load(os.path.join(train, f"{kind}_{i}.pkl")) for i in range(motion_ref.SPLIT)]
        assert [len(p) for p in parts] == list(g[f"train_{kind}_counts"])
        assert [k for p in parts for k in p] == list(g[f"train_{kind}_ids"])
        for p in parts:
            for k, obj in p.items():
                _same_track(obj, tr_tracks[k])
    # val: split by the prediction — exact on every row outside the band the reference's own stop leaves open
    w, b = motion.load_model(os.path.join(val, "motion_svm.json"))
    ref = g["decision"]
    d = g["valX"] @ w + b
    err = np.abs(d - ref) / (1 + np.abs(ref))
    print(f"cli model: max |d - d_ref| / (1 + |d_ref|) = {err.max():.3e}")
    assert err.max() <= 1e-3
    band = set(g["val_keep_ids"][np.abs(ref) <= 2e-3])
    assert len(band) <= 0.01 * len(ref)
    got = {kind: _load(os.path.join(val, f"{kind}.pkl")) for kind in ("trackStatic", "trackDynamic")}
    for kind in got:
        assert [k for k in got[kind] if k not in band] == [k for k in g[f"val_{kind}_ids"] if k not in band]
        for k, obj in got[kind].items():
            _same_track(obj, va_tracks[k])
    assert sorted(list(got["trackStatic"]) + list(got["trackDynamic"])) == sorted(g["val_keep_ids"])
    if not band:                                            # then the prediction is the reference's row for row: the same lines
        assert out == str(g["printed"])


def test_model_option_classifies_with_the_recorded_model(dirs, tmp_path, capsys):
    g = golden("motion")
    train, val = dirs["train"][0], dirs["val"][0]
    path = str(tmp_path / "recorded.json")
    motion.save_model(path, g["coef"], float(g["intercept"][0]))
    motion.main(["--track_train", train, "--track_val", val, "--split", "16", "--model", path])
    out = capsys.readouterr().out
    band = set(g["val_keep_ids"][np.abs(g["decision"]) <= 2e-3])
    for kind in ("trackStatic", "trackDynamic"):
        got = _load(os.path.join(val, f"{kind}.pkl"))
        assert [k for k in got if k not in band] == [k for k in g[f"val_{kind}_ids"] if k not in band]
    if not band:
        assert f"Score on test set: {g['score_text']}" in out
    assert motion.load_model(os.path.join(val, "motion_svm.json"))[0].tolist() == g["coef"].tolist()
