"""The baseline command lines (python -m 3dal_pytorch_amd.baseline static / dynamic / labels) on the seeded work dir of
tests/baseline_ref.py, against what the reference's tools/static_init.py, tools/dynamic_init.py and tools/eval.py printed
and wrote on the same files (tests/golden/baseline.npz; the IoU of a pair there is tests/iou_ref.py's).

The `[Init]` / `[Static]` lines are compared as text: the device IoU is within 1e-5 of the oracle's and the generator
asserts that every printed .4f value keeps 2e-5 from a rounding point and every sample 1e-5 from its threshold. The two
`mIOU of ...` lines print a float32 mean with all its digits, which 1e-5 per IoU does move: their text up to the number
is compared, and the number to 1e-5 (a mean moves by no more than its terms)."""
import importlib
import os
import pickle
import re

import numpy as np
import pytest

import baseline_ref
from _common import golden

baseline = importlib.import_module("3dal_pytorch_amd.baseline")
pytestmark = pytest.mark.gpu
TOL = 1e-5                      # the bound tests/test_gpu_iou.py holds the IoU kernels to against iou_ref


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    g = golden("baseline")
    root = str(tmp_path_factory.mktemp("baseline_files"))
    paths, c = baseline_ref.write_work_dir(root, int(g["seed"]))
    return g, root, paths, c


def test_static_command_prints_the_reference_lines_and_writes_its_pickle(work, capsys):
    g, root, paths, c = work
    assert not os.path.exists(os.path.join(root, "static"))               # created by the run (the reference fails)
    capsys.readouterr()
    baseline.main(["static", "--track", paths["static"], "--infos", paths["infos"], "--det_annos", paths["det_annos"]])
    out = capsys.readouterr().out
    assert out == str(g["static_lines"])
    with open(os.path.join(root, "static", "static.pkl"), "rb") as f:
        got = pickle.load(f)
    before = sorted(c["det_annos"], key=lambda d: d["frame_id"])
    assert [d["frame_id"] for d in got] == list(g["pkl_frame_ids"])
    assert all(list(d.keys()) == list(g["pkl_keys"]) for d in got)
    off = g["pkl_offsets"]
    assert [len(d["boxes_lidar"]) for d in got] == list(np.diff(off))
    assert all(d["boxes_lidar"].dtype == np.float32 and d["score"].dtype == np.float32 for d in got)
    score = np.concatenate([d["score"] for d in got])
    boxes = np.concatenate([d["boxes_lidar"] for d in got])
    assert np.array_equal(score, g["pkl_score"])                           # exactly
    changed = np.concatenate([np.any(d["boxes_lidar"] != b["boxes_lidar"], axis=1) | (d["score"] != b["score"])
                              for d, b in zip(got, before)])
    want_changed = g["pkl_rewritten"]
    assert np.array_equal(changed, want_changed) and 0 < changed.sum() < len(changed)      # the SAME rows rewritten
    assert np.array_equal(boxes[~changed].view(np.uint32), g["pkl_boxes"][~changed].view(np.uint32))
    want = g["pkl_boxes"][changed]
    err = np.abs(boxes[changed].astype(np.float64) - want) / np.maximum(1.0, np.abs(want).max(axis=1, keepdims=True))
    print(f"static.pkl: {int(changed.sum())} rewritten rows, max scaled error {err.max():.3e}")
    assert err.max() <= 4e-6
    assert all(np.array_equal(d["name"], b["name"]) and d["metadata"] == b["metadata"] for d, b in zip(got, before))


def test_dynamic_command_prints_the_reference_lines(work, capsys):
    g, _, paths, _ = work
    capsys.readouterr()
    baseline.main(["dynamic", "--track", paths["dynamic"], "--infos", paths["infos"]])
    assert capsys.readouterr().out == str(g["dynamic_lines"])


def test_labels_command_prints_the_reference_lines(work, capsys):
    g, _, paths, _ = work
    capsys.readouterr()
    baseline.main(["labels", "--track", paths["static"], "--infos", paths["infos"], "--static", paths["labels"]])
    got, want = capsys.readouterr().out.splitlines(), str(g["labels_lines"]).splitlines()
    assert got[:3] == want[:3] and len(got) == len(want) == 5
    for a, b, ref in zip(got[3:], want[3:], g["lab_miou"]):
        head, value = re.fullmatch(r"(.*: )(\S+)", a).groups()
        assert head == re.fullmatch(r"(.*: )(\S+)", b).group(1) and "\033[94mInfo\033[0m" in head
        print(f"{head[-16:]}{value} (reference {ref})")
        assert abs(float(value) - float(ref)) <= TOL
    r = baseline.run_labels(paths["static"], paths["infos"], paths["labels"])
    capsys.readouterr()
    assert r["iou_track"].dtype == np.float32 and np.abs(r["iou_track"] - g["lab_iou_track"]).max() <= TOL
    assert np.abs(r["iou_static"] - g["lab_iou_static"]).max() <= TOL


def test_a_scored_sample_without_its_detection_row_raises_the_reference_assertion(tmp_path):
    paths, _ = baseline_ref.write_work_dir(str(tmp_path), int(golden("baseline")["seed"]), break_row=True)
    with pytest.raises(AssertionError, match="Bounding box not in det_annos."):
        baseline.run_static(paths["static"], paths["infos"], paths["det_annos"])
    assert not os.path.exists(os.path.join(str(tmp_path), "static", "static.pkl"))
