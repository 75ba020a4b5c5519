"""The training run's host side without a GPU: the decode of the box metric against the reference's own
compute_box3d_iou (tests/golden/train_metrics.npz, tests/golden/gen_train_metrics.py), the train / validation split
against the reference's preprocessing, the drop-in `utils` module the reference's drivers import, and the C ABI entry
of the metric kernel."""
import importlib
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from _common import ROOT, golden

metrics = importlib.import_module("3dal_pytorch_amd.metrics")
fit = importlib.import_module("3dal_pytorch_amd.fit")
ev = importlib.import_module("3dal_pytorch_amd.eval")
_hip = importlib.import_module("3dal_pytorch_amd._hip")

_FIELDS = ("center", "heading_scores", "heading_residuals", "size_scores", "size_residuals", "center_label",
           "heading_class_label", "heading_residual_label", "size_class_label", "size_residual_label")


def test_numpy_decode_equals_the_reference_decode():
    """the boxes the reference hands to its geometry, bit for bit: ties, angles just above pi, every size class"""
    g = golden("train_metrics")
    pred, label = metrics.decode_boxes_numpy(*[g[k] for k in _FIELDS])
    assert np.array_equal(pred, g["pred_box"])
    assert np.array_equal(label, g["label_box"])
    assert (g["pred_box"][:, 6] > np.pi - 0.6).any() and len(np.unique(np.argmax(g["size_scores"], 1))) == 3


def test_numpy_decode_out_of_range_labels_give_nan():
    g = golden("train_metrics")
    args = [g[k].copy() for k in _FIELDS]
    args[6][:3] = [-1, 12, 99]
    args[8][3:5] = [3, -2]
    _, label = metrics.decode_boxes_numpy(*args)
    assert np.isnan(label[:3, 6]).all() and np.isnan(label[3:5, 3:6]).all()
    assert np.isfinite(label[5:]).all()


def _track_set(tmp_path, g):
    track, infos = {}, {}
    for k, key in enumerate(g["track_keys"]):
        key = str(key)
        tokens = [f"{key}_f{j}" for j in range(g["track_scores"].shape[1])]
        track[key] = {"score": [np.float32(s) for s in g["track_scores"][k]], "token": tokens, "match": ["x", f"obj_{key}"]}
        for j, tok in enumerate(tokens):
            objs = [{"name": "other", "box": np.zeros(9, np.float32)}]
            if g["track_has_gt"][k, j]:
                objs.append({"name": f"obj_{key}", "box": np.ones(9, np.float32)})
            path = os.path.join(tmp_path, tok + ".pkl")
            with open(path, "wb") as fh:
                pickle.dump({"veh_to_global": np.eye(4).reshape(16), "objects": objs}, fh)
            infos[tok] = {"anno_path": path, "token": tok}
    return track, infos


def test_split_equals_the_reference_preprocessing(tmp_path):
    g = golden("train_metrics")
    track, infos = _track_set(tmp_path, g)
    ev.fix_seed(fit.SEED)
    tr, va = fit.split_tracks(dict(track), ev.Annos(infos))
    assert list(tr) == list(g["static_train_keys"]) and list(va) == list(g["static_val_keys"])
    ev.fix_seed(fit.SEED)
    tr, va = fit.split_tracks(dict(track))
    assert list(tr) == list(g["dynamic_train_keys"]) and list(va) == list(g["dynamic_val_keys"])


def test_lr_schedule_is_the_references():
    f = fit.lr_lambda(0.001)
    assert [f(e) for e in (0, 19, 20, 39, 40)] == [1.0, 1.0, 0.7, 0.7, 0.7 ** 2]
    assert f(20 * 40) == 0.01                               # 0.001 * 0.7^40 < 1e-5: the floor


def test_drivers_utils_imports_resolve_in_the_dropin():
    """the exact `from utils import` lines of static_train.py:16, dynamic_train.py:16, static_eval.py:11-13 and
    dynamic_eval.py:11-13, in a fresh process with dropin/ first on sys.path and no GPU"""
    dropin = os.path.join(ROOT, "3dal_pytorch_amd", "dropin")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from utils import fixSeed, create_logger, reorganize_info, compute_box3d_iou\n"
            "from utils import class2angle, class2size, compute_box3d_iou\n"
            "from utils import fixSeed, create_logger, reorganize_info\n"
            "from utils import size2class, angle2class\n"
            "from utils import NUM_HEADING_BIN, NUM_SIZE_CLUSTER, MEAN_SIZE_ARR\n"
            "import utils, numpy as np\n"
            "assert utils.__file__.startswith(sys.path[0])\n"
            "assert class2angle(6, 0.1, NUM_HEADING_BIN) == 6 * (2 * np.pi / 12.0) + 0.1 - 2 * np.pi\n"
            "assert class2angle(1, 0.1, NUM_HEADING_BIN) == 2 * np.pi / 12.0 + 0.1\n"
            "assert np.array_equal(class2size(2, np.zeros(3)), MEAN_SIZE_ARR[2])\n"
            "c, r = size2class(np.array([9.0, 2.5, 3.0])); assert c == 1 and np.allclose(r, [-1.0, -0.1, -0.2])\n"
            "assert angle2class(0.1, 12)[0] == 0 and reorganize_info([{'token': 't'}]) == {'t': {'token': 't'}}\n"
            "print('ok')" % dropin)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp", env=env)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_metric_entry_in_the_c_abi():
    with open(os.path.join(ROOT, "include", "dal3.h")) as f:
        h = f.read()
    assert "int dal3_box_estimation_metrics(const dal3_box_metric_args* args, dal3_stream stream);" in h
    assert "#define DAL3_VERSION 170" in h
    assert "dal3_box_estimation_metrics" in _hip.SIGNATURES
    assert _hip.BoxMetricArgs.acc.offset == 272 and _hip.BoxMetricArgs.f64_fields.offset == 176


@pytest.mark.parametrize("argv", [["static", "--track", "d", "--infos", "i", "--precision", "bf16"],
                                  ["static", "--track", "d", "--infos", "i", "--sampler", "host"]])
def test_command_line_refuses_what_it_cannot_run(argv):
    with pytest.raises(SystemExit):
        fit.main(argv)
