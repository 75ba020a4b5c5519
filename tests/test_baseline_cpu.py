"""CPU-side checks of the baseline runs (3dal_pytorch_amd/baseline.py; dal3_score_tracks / dal3_best_gt_iou): the sample
recipe against what the reference's tools/static_init.py, tools/dynamic_init.py and tools/eval.py recorded
(tests/golden/baseline.npz, written by tests/golden/gen_baseline.py), the host flattening, the C ABI's entries and
argument checks, and the code object's scratch use. No GPU compute here."""
import ctypes
import importlib
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

import baseline_ref
import iou_ref
from _common import ROOT, golden

graft_entry = importlib.import_module("__graft_entry__")
hip = importlib.import_module("3dal_pytorch_amd._hip")
ev = importlib.import_module("3dal_pytorch_amd.eval")
baseline = importlib.import_module("3dal_pytorch_amd.baseline")

CSRC = os.path.join(ROOT, "3dal_pytorch_amd", "csrc")


def _work_dir(tmp_path):
    g = golden("baseline")
    paths, c = baseline_ref.write_work_dir(str(tmp_path), int(g["seed"]))
    s = (sum(float(np.sum(np.vstack(v["bbox"]))) for t in (c["static"], c["dynamic"]) for v in t.values())
         + sum(float(o["box"].astype(np.float64).sum()) for f in c["frames"] for o in f["objects"])
         + sum(float(f["rows"].astype(np.float64).sum()) for f in c["frames"]))
    assert abs(s - float(g["in_sum"])) < 1e-6, "the seeded work dir drifted from the fixture"
    return g, paths, c


def _tracks(c, name):
    annos = baseline_ref.annos_of(c["frames"])
    track = c["dynamic"] if name == "dynamic_init" else baseline_ref.drop_tracks_without_best_gt(c["static"], annos)
    return track, annos


@pytest.mark.parametrize("name", baseline_ref.FLAVOURS)
def test_restated_recipe_reproduces_the_reference_boxes_and_sums(tmp_path, name):
    """baseline_ref.samples — one NumPy step per sample — gives the boxes the reference handed to get_3d_box, and
    iou_ref.paired on them the means the reference's own loops returned."""
    g, _, c = _work_dir(tmp_path)
    track, annos = _tracks(c, name)
    s = baseline_ref.samples(track, annos, best=(name == "static_best"))
    assert s["pred"].shape == g[f"{name}_pred"].shape and s["n_samples"] == int(g[f"{name}_n_samples"])
    np.testing.assert_allclose(s["pred"], g[f"{name}_pred"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(s["label"], g[f"{name}_label"], rtol=0, atol=1e-9)
    assert np.all(g[f"{name}_pred"][:, 6] == 0.0)
    bev, v3 = iou_ref.paired(g[f"{name}_pred"], g[f"{name}_label"])
    np.testing.assert_allclose(bev, g[f"{name}_iou_bev"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(v3, g[f"{name}_iou_3d"], rtol=0, atol=1e-12)
    n = s["n_samples"]
    thr = baseline_ref.thresholds(s["types"][s["has_gt"]])
    n_pass = int(np.sum(v3.astype(np.float32) >= thr.astype(np.float32)))
    assert n_pass == int(g[f"{name}_n_pass"])
    # the reference adds float32 values (in float32 with today's NumPy): 180 samples keep that within 2e-6 of float64 sums
    np.testing.assert_allclose([bev.astype(np.float32).sum(dtype=np.float64) / n, v3.astype(np.float32).sum(dtype=np.float64) / n,
                                n_pass / n], g[f"{name}_means"], rtol=0, atol=2e-6)
    lines = str(g["dynamic_lines" if name == "dynamic_init" else "static_lines"])
    tag = "Static" if name == "static_best" else "Init"
    assert f"[{tag}] Box IoU (2D/3D): {bev.astype(np.float32).sum(dtype=np.float64) / n:.4f}/{v3.astype(np.float32).sum(dtype=np.float64) / n:.4f}\n" in lines
    assert f"[{tag}] Box estimation accuracy: {n_pass / n:.4f}\n" in lines


@pytest.mark.parametrize("name", baseline_ref.FLAVOURS)
def test_flatten_gives_the_fixtures_samples(tmp_path, name):
    """baseline.flatten on the work dir's files: the reference's sample order, n_samples, has_gt, types and best rows
    exactly; and its tables, put through the restated recipe row by row, give the recorded boxes."""
    g, paths, c = _work_dir(tmp_path)
    with open(paths["infos"], "rb") as f:
        annos = ev.Annos(ev.reorganize_info(pickle.load(f)))
    with open(paths["dynamic" if name == "dynamic_init" else "static"], "rb") as f:
        track = pickle.load(f)
    if name != "dynamic_init":
        track = ev.preprocessing(track, annos)
    flat = baseline.flatten(track, annos)
    assert flat["n_samples"] == int(g[f"{name}_n_samples"])
    assert np.array_equal(flat["has_gt"].astype(bool), g[f"{name}_has_gt"])
    assert np.array_equal(flat["types"], g[f"{name}_types"]) and flat["types"].dtype == np.int32
    assert np.array_equal(flat["best_row"], g[f"{name}_best_row"])
    assert np.array_equal(flat["own_row"], np.arange(flat["n_samples"]))
    assert flat["gt"].dtype == np.float32 and flat["boxes"].dtype == np.float64 and flat["pose_inv"].shape[1] == 16
    assert len(annos._cache) == len(flat["tokens"])                      # every pickle read once
    rows = flat["best_row"] if name == "static_best" else flat["own_row"]
    pred, label = [], []
    for s in np.nonzero(flat["has_gt"])[0]:
        init = baseline_ref.transform_box(flat["boxes"][rows[s]][np.newaxis], flat["pose_inv"][flat["frame"][s]].reshape(4, 4))[0]
        gt = flat["gt"][s]
        pred.append(np.concatenate([init[:3], baseline_ref.size_round_trip(init[3:6]), [0.0]]))
        label.append(np.concatenate([gt[:3].astype(np.float64), baseline_ref.size_round_trip(gt[3:6]),
                                     [baseline_ref.angle_round_trip(gt[6] - init[6])]]))
    np.testing.assert_allclose(np.array(pred), g[f"{name}_pred"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.array(label), g[f"{name}_label"], rtol=0, atol=1e-9)
    tracks = list(track.values())
    assert [float(x) for x in flat["max_score"]] == [float(np.max(v["score"])) for v in tracks]
    assert np.array_equal(flat["track_first"], np.cumsum([0] + [len(v["token"]) for v in tracks]))


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dal3.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ("dal3_score_workspace_bytes", "dal3_score_tracks", "dal3_best_gt_iou"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    assert hip.lib().dal3_version() == graft_entry.header_version()
    # one slab entry per 256 samples
    assert hip.lib().dal3_score_workspace_bytes(0) == 0
    assert hip.lib().dal3_score_workspace_bytes(256) * 2 == hip.lib().dal3_score_workspace_bytes(257)
    assert hip.lib().dal3_score_workspace_bytes(1 << 20) == 4096 * hip.lib().dal3_score_workspace_bytes(1)


def _score_args(**kw):
    fake = 0x1000                                                        # never dereferenced: every call fails before a launch
    a = hip.ScoreArgs()
    a.S, a.R, a.F = 5, 5, 2
    for name in ("boxes", "box_row", "frame", "pose_inv", "gt", "has_gt", "type", "iou_3d"):
        setattr(a, name, fake)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _best_args(**kw):
    a = hip.BestGtArgs()
    a.Q, a.F, a.G = 3, 2, 9
    for name in ("queries", "query_frame", "gt_offsets", "gt_boxes", "best_iou_3d"):
        setattr(a, name, 0x1000)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_errors_without_a_gpu():
    lib = hip.lib()
    big = (1 << 24) + 1
    assert lib.dal3_score_tracks(None, None) == hip.EINVAL and b"null args" in lib.dal3_last_error()
    assert lib.dal3_best_gt_iou(None, None) == hip.EINVAL and b"null args" in lib.dal3_last_error()
    cases = [
        (lib.dal3_score_tracks, _score_args(S=-1), b"bad S / R / F"),
        (lib.dal3_score_tracks, _score_args(S=big), b"DAL3_MAX_ITEMS"),
        (lib.dal3_score_tracks, _score_args(F=-2), b"bad S / R / F"),
        (lib.dal3_score_tracks, _score_args(gt_f64=2), b"gt_f64"),
        (lib.dal3_score_tracks, _score_args(max_workgroups=-1), b"max_workgroups"),
        (lib.dal3_score_tracks, _score_args(iou_3d=None), b"no accumulator and no output"),
        (lib.dal3_score_tracks, _score_args(box_row=None), b"null per-sample table"),
        (lib.dal3_score_tracks, _score_args(has_gt=None), b"null per-sample table"),
        (lib.dal3_score_tracks, _score_args(boxes=None), b"null boxes"),
        (lib.dal3_score_tracks, _score_args(gt=None), b"null boxes"),
        (lib.dal3_score_tracks, _score_args(acc=0x1000), b"needs a workspace"),
        (lib.dal3_best_gt_iou, _best_args(Q=-1), b"bad Q / F / G"),
        (lib.dal3_best_gt_iou, _best_args(Q=big), b"DAL3_MAX_ITEMS"),
        (lib.dal3_best_gt_iou, _best_args(boxes_f64=3), b"boxes_f64"),
        (lib.dal3_best_gt_iou, _best_args(best_iou_3d=None), b"no output"),
        (lib.dal3_best_gt_iou, _best_args(queries=None), b"null queries"),
        (lib.dal3_best_gt_iou, _best_args(gt_boxes=None), b"null queries"),
    ]
    for fn, args, word in cases:
        assert fn(args, None) == hip.EINVAL, word
        assert word in lib.dal3_last_error(), (word, lib.dal3_last_error())
    need = lib.dal3_score_workspace_bytes(5)
    assert lib.dal3_score_tracks(_score_args(acc=0x1000, workspace=0x1000, workspace_bytes=need - 1), None) == hip.EWORKSPACE
    assert b"dal3_score_workspace_bytes" in lib.dal3_last_error()
    assert lib.dal3_score_workspace_bytes(-1) == 0 and lib.dal3_score_workspace_bytes(big) == 0
    # nothing to do is not an error and launches nothing (no GPU needed)
    assert lib.dal3_score_tracks(_score_args(S=0, box_row=None, gt=None), None) == 0
    assert lib.dal3_score_tracks(_score_args(S=0, acc=0x1000), None) == 0
    assert lib.dal3_best_gt_iou(_best_args(Q=0, queries=None, best_iou_3d=None), None) == 0


def test_score_kernels_use_no_scratch_and_no_float_atomics(tmp_path):
    """.private_segment_fixed_size is 0 for every kernel of dal3_score.hip, and neither the source nor the code object
    holds a floating-point atomic (the sums have one order: include/dal3.h)."""
    out = tmp_path / "score.s"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
                    "--cuda-device-only", "-S", os.path.join(CSRC, "dal3_score.hip"), "-o", str(out)], check=True)
    text = out.read_text()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(kernels) == 4 and sum("score_tracks" in k for k in kernels) == 1 and sum("best_gt_iou" in k for k in kernels) == 2, kernels
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"atomic_(add|pk_add|fadd|fmin|fmax|min|max)_(f|pk_)", text), "a floating-point atomic in the code object"
    src = open(os.path.join(CSRC, "dal3_score.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code.lower() and "asm" not in code
    assert "#pragma clang fp contract(off)" in src and '#include "dal3_iou_pair.h"' in src
    assert "dal3_score.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_command_line_refuses_unknown_runs_and_missing_arguments(capsys):
    for argv in (["refine"], [], ["static", "--track", "a.pkl", "--infos", "b.pkl"], ["dynamic", "--track", "a.pkl"],
                 ["labels", "--track", "a.pkl", "--infos", "b.pkl"], ["dynamic", "--track", "a", "--infos", "b", "--det_annos", "c"]):
        with pytest.raises(SystemExit) as e:
            baseline.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def test_writeback_plan_keeps_its_default_and_checks_pose_best():
    """post.WritebackPlan's new optional argument: refused for the dynamic write-back and for a wrong shape before
    anything touches a device"""
    post = importlib.import_module("3dal_pytorch_amd.post")
    tracks = [{"token": ["a"], "score": [np.float32(1)], "bbox": [np.zeros(7)]}]
    with pytest.raises(ValueError, match="static"):
        post.WritebackPlan(tracks, {"a": np.eye(4).reshape(16)}, {(0, "a"): True}, {"a": np.zeros((1, 7), np.float32)},
                           static=False, pose_best=np.eye(4).reshape(1, 16))
    with pytest.raises(ValueError):
        post.WritebackPlan(tracks, {"a": np.eye(4).reshape(16)}, {(0, "a"): True}, {"a": np.zeros((1, 7), np.float32)},
                           static=True, pose_best=np.zeros((3, 16)))
