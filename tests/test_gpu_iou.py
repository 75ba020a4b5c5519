"""Rotated-box IoU on the MI355X (3dal_pytorch_amd/iou.py -> dal3_box_iou_*): against the float64 oracle
tests/iou_ref.py, pairwise vs paired bit for bit, translation invariance, empty and non-finite inputs; the eval
metrics (eval.box_metrics) against the reference's postprocessing fixture; eval.run's two [Eval] lines."""
import importlib
import pickle
import re

import numpy as np
import pytest
import torch

import iou_ref
from _common import golden, synth

iou = importlib.import_module("3dal_pytorch_amd.iou")
ev = importlib.import_module("3dal_pytorch_amd.eval")
pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"


def scene_boxes(n, seed, extent=150.0):
    """n vehicle-like boxes scattered over an extent x extent area, about as dense as a busy lidar scene: most pairs
    are far apart, a few overlap"""
    rng = np.random.default_rng(seed)
    size = np.array(synth.arch.MEAN_SIZE)[rng.integers(0, 3, n)] * rng.uniform(0.8, 1.2, (n, 3))
    return np.concatenate([rng.uniform(-extent / 2, extent / 2, (n, 2)), rng.normal(0, 0.5, (n, 1)), size,
                           rng.uniform(-np.pi, np.pi, (n, 1))], 1)


def designed():
    pi = np.pi
    rows = [([0, 0, 0, 4, 2, 1.5, 0.3], [0, 0, 0, 4, 2, 1.5, 0.3]), ([0, 0, 0, 4, 2, 1, 0], [0, 0, 0, 2, 1, 1, 0]),
            ([0, 0, 0, 2, 2, 1, 0], [1, 0, 0, 2, 2, 1, 0]), ([0, 0, 0, 2, 2, 1, 0], [2, 0, 0, 2, 2, 1, 0]),
            ([0, 0, 0, 2, 2, 1, 0], [0, 0, 0, 2, 2, 1, pi / 2]), ([0, 0, 0, 4, 1, 1, 0], [0, 0, 0, 4, 1, 1, pi / 2]),
            ([3, -2, 0, 4.8, 1.8, 1.5, 0.7], [3, -2, 0, 4.8, 1.8, 1.5, 0.7 + pi]),
            ([0, 0, 0, 10, 0.2, 1, 0.0], [0.5, 0.05, 0, 10, 0.2, 1, 0.01]),
            ([0, 0, 0, 4, 2, 1, 0.25], [0.3, 0.2, 0.4, 4, 2, 1, 0.25]), ([0, 0, 0, 4, 2, 1, 0], [10, 10, 0, 4, 2, 1, 1.0]),
            ([0, 0, 0, 0, 2, 1, 0], [0, 0, 0, 0, 2, 1, 0]), ([0, 0, 0, 4, 2, 0, 0], [0, 0, 0, 4, 2, 1, 0])]
    return np.array([r[0] for r in rows], float), np.array([r[1] for r in rows], float)


def near_pairs(n, seed):
    """pairs that mostly overlap (the oracle's reference-fixture distribution)"""
    rng = np.random.default_rng(seed)
    a = scene_boxes(n, seed, 100.0)
    b = np.concatenate([a[:, :2] + rng.normal(0, 1, (n, 2)) * a[:, 3:5] * 0.5, a[:, 2:3] + rng.normal(0, 0.3, (n, 1)),
                        a[:, 3:6] * rng.uniform(0.7, 1.3, (n, 3)), a[:, 6:7] + rng.normal(0, 0.5, (n, 1))], 1)
    return a, b


def gpu(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=DEV, dtype=dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pairwise_scene_4096_vs_oracle(dtype):
    a, b = scene_boxes(4096, 1), scene_boxes(4096, 2)
    a_in, b_in = gpu(a, dtype), gpu(b, dtype)
    bev, v3 = iou.boxes_iou_bev_3d(a_in, b_in)
    want_b, want_3 = iou_ref.pairwise(a_in.double().cpu().numpy(), b_in.double().cpu().numpy())
    bev, v3 = bev.cpu().numpy(), v3.cpu().numpy()
    assert (want_b > 0).sum() > 1000 and (want_b > 0).mean() < 0.01          # scene-like: few pairs overlap
    assert np.abs(bev - want_b).max() <= TOL and np.abs(v3 - want_3).max() <= TOL
    assert np.array_equal(bev == 0, want_b == 0) or np.abs(bev[want_b == 0]).max() <= TOL
    assert torch.equal(iou.boxes_iou_bev(a_in, b_in).cpu(), torch.from_numpy(bev))     # one output or both: same bits
    assert torch.equal(iou.boxes_iou3d(a_in, b_in).cpu(), torch.from_numpy(v3))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_paired_and_designed_vs_oracle(dtype):
    da, db = designed()
    na, nb = near_pairs(30000, 3)
    a, b = np.concatenate([da, na]), np.concatenate([db, nb])
    a_in, b_in = gpu(a, dtype), gpu(b, dtype)
    bev, v3 = (x.cpu().numpy() for x in iou.paired_iou(a_in, b_in))
    want_b, want_3 = iou_ref.paired(a_in.double().cpu().numpy(), b_in.double().cpu().numpy())
    assert np.abs(bev - want_b).max() <= TOL, np.argmax(np.abs(bev - want_b))
    assert np.abs(v3 - want_3).max() <= TOL, np.argmax(np.abs(v3 - want_3))
    assert bev[0] == 1.0 and bev[3] == 0.0 and bev[9] == 0.0 and bev[10] == 0.0 and v3[11] == 0.0
    pw_b, pw_3 = (x.cpu().numpy() for x in iou.boxes_iou_bev_3d(a_in[:len(da)], b_in[:len(db)]))
    assert np.abs(np.diag(pw_b) - want_b[:len(da)]).max() <= TOL


@pytest.mark.parametrize("n,m", [(1, 1), (1, 200), (200, 1), (63, 63), (64, 64), (65, 65), (17, 129), (33, 191),
                                 (16, 64), (15, 65)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_ragged_shapes(n, m, dtype):
    a, b = near_pairs(max(n, m), 4)
    a, b = a[:n], b[:m]
    a[:, :2] = b[np.arange(n) % m, :2] + 0.5                                  # every row overlaps something
    a_in, b_in = gpu(a, dtype), gpu(b, dtype)
    bev, v3 = (x.cpu().numpy() for x in iou.boxes_iou_bev_3d(a_in, b_in))
    assert bev.shape == (n, m)
    want_b, want_3 = iou_ref.pairwise(a_in.double().cpu().numpy(), b_in.double().cpu().numpy())
    assert np.abs(bev - want_b).max() <= TOL and np.abs(v3 - want_3).max() <= TOL
    assert (want_b > 0).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pairwise_is_bit_identical_to_paired(dtype):
    a, b = near_pairs(300, 5)
    a_in, b_in = gpu(a, dtype), gpu(b[:130], dtype)
    bev, v3 = iou.boxes_iou_bev_3d(a_in, b_in)
    i, j = torch.meshgrid(torch.arange(300), torch.arange(130), indexing="ij")
    pb, p3 = iou.paired_iou(a_in[i.reshape(-1).to(DEV)], b_in[j.reshape(-1).to(DEV)])
    assert (bev > 0).float().mean() > 0.005
    assert torch.equal(bev.reshape(-1).view(torch.int32), pb.view(torch.int32))
    assert torch.equal(v3.reshape(-1).view(torch.int32), p3.view(torch.int32))


def test_translation_invariance_in_float64():
    """the same pairs 1e4 m away (float64 input): the differences are taken in float64, so the IoU does not move. The
    reference's fp32 absolute-frame arithmetic gives 0.99995 for two identical boxes at (5000.3, -3000.7)."""
    da, db = designed()
    na, nb = near_pairs(20000, 6)
    a, b = np.concatenate([da, na]), np.concatenate([db, nb])
    shift = np.array([1e4, -1e4, 0, 0, 0, 0, 0])
    b0, v0 = iou.paired_iou(gpu(a, torch.float64), gpu(b, torch.float64))
    b1, v1 = iou.paired_iou(gpu(a + shift, torch.float64), gpu(b + shift, torch.float64))
    assert (b0 - b1).abs().max().item() <= 1e-6 and (v0 - v1).abs().max().item() <= 1e-6
    far = np.array([[5000.3, -3000.7, 1, 4.8, 1.8, 1.5, 0.2]])
    assert iou.paired_iou(gpu(far, torch.float64), gpu(far, torch.float64))[0].item() == 1.0


def test_empty_inputs():
    e = torch.zeros((0, 7), device=DEV)
    x = torch.tensor([[0, 0, 0, 4, 2, 1, 0.0]], device=DEV)
    assert iou.boxes_iou_bev(e, x).shape == (0, 1) and iou.boxes_iou3d(x, e).shape == (1, 0)
    assert iou.boxes_iou_bev(e, e).shape == (0, 0)
    pb, p3 = iou.paired_iou(e, e)
    assert pb.shape == (0,) and p3.shape == (0,) and pb.dtype == torch.float32


def test_non_finite_inputs_poison_only_their_row_and_column():
    a, b = near_pairs(70, 7)
    a[:, :2] = b[:, :2] + 0.3
    a[5, 0], a[40, 6], b[9, 4], b[66, 2] = np.nan, np.inf, -np.inf, np.nan
    bev, v3 = (x.cpu().numpy() for x in iou.boxes_iou_bev_3d(gpu(a, torch.float32), gpu(b, torch.float32)))
    bad_r, bad_c = np.zeros(70, bool), np.zeros(70, bool)
    bad_r[[5, 40]], bad_c[[9, 66]] = True, True
    mask = bad_r[:, None] | bad_c[None, :]
    assert np.isnan(bev[mask]).all() and np.isnan(v3[mask]).all()
    assert np.isfinite(bev[~mask]).all() and np.isfinite(v3[~mask]).all()
    assert (bev[~mask] > 0).any()


def test_inputs_are_checked():
    x = torch.zeros((3, 7), device=DEV)
    with pytest.raises(RuntimeError):
        iou.boxes_iou_bev(x.cpu(), x)
    with pytest.raises(ValueError):
        iou.boxes_iou_bev(x[:, :6], x)
    with pytest.raises(TypeError):
        iou.paired_iou(x.half(), x.half())
    with pytest.raises(TypeError):
        iou.paired_iou(x, x.double())
    with pytest.raises(ValueError):
        iou.paired_iou(x, x[:2])


@pytest.mark.parametrize("head", ["static", "dynamic"])
def test_box_metrics_reproduce_the_reference_numbers(tmp_path, head):
    g = golden("eval_metrics")
    paths, *_ = synth.segment_files(str(tmp_path), int(g["segment_seed"]), n_frames=int(g["segment_n_frames"]),
                                    n_tracks=int(g["segment_n_tracks"]))
    annos = ev.Annos(ev.reorganize_info(pickle.load(open(paths["infos"], "rb"))))
    track = pickle.load(open(paths[head], "rb"))
    if head == "static":
        track = ev.preprocessing(track, annos)
    m = ev.box_metrics(track, annos, g[f"{head}_final"], static=(head == "static"))
    assert m["n_samples"] == int(g[f"{head}_n_samples"])
    assert np.abs(m["iou_3d"] - g[f"{head}_iou_3d"]).max() <= TOL
    for k in ("iou2d", "iou3d", "acc"):
        assert abs(m[k] - float(g[f"{head}_{k}"])) <= 1e-6, (k, m[k], float(g[f"{head}_{k}"]))
    assert m["n_correct"] == round(float(g[f"{head}_acc"]) * m["n_samples"])
    assert m["n_other_type"] == 0


@pytest.mark.parametrize("head", ["static", "dynamic"])
def test_eval_run_logs_the_two_lines(tmp_path, head):
    paths, tracks, *_ = synth.segment_files(str(tmp_path), 77, n_frames=12, n_tracks=7)
    kind = "static_one" if head == "static" else "dynamic"
    sd = synth.state_dict(kind)
    ckpt = str(tmp_path / f"{kind}.pth")
    torch.save({"epoch": 1, "model_state_dict": {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}}, ckpt)
    out = ev.run(head, paths[head], paths["infos"], paths["det_annos"], ckpt, batch_size=8, sampler="device")
    assert isinstance(out, tuple) and len(out) == 2
    final, det_annos = out
    n = len(ev.preprocessing(pickle.load(open(paths["static"], "rb")), ev.Annos(ev.reorganize_info(
        pickle.load(open(paths["infos"], "rb")))))) if head == "static" else sum(len(t["token"]) for t in tracks)
    assert isinstance(final, np.ndarray) and final.shape == (n, 7) and final.dtype == np.float64
    result = tmp_path / head / "box" / ("one_box_est.pkl" if head == "static" else "box.pkl")
    saved = pickle.load(open(result, "rb"))
    assert all(np.array_equal(s["boxes_lidar"], d["boxes_lidar"]) for s, d in zip(saved, det_annos))
    log = (tmp_path / head / "log" / "eval" / ("one_box_est.txt" if head == "static" else "eval.txt")).read_text()
    lines = log.splitlines()
    k = next(i for i, line in enumerate(lines) if "Saving results to" in line)
    assert "[Eval] Box IoU (2D/3D): " in lines[k + 1] and "[Eval] Box estimation accuracy: " in lines[k + 2]
    assert re.search(r"\[Eval\] Box IoU \(2D/3D\): (\d\.\d{4}|nan)/(\d\.\d{4}|nan)$", lines[k + 1]), lines[k + 1]
    assert re.search(r"\[Eval\] Box estimation accuracy: (\d\.\d{4}|nan)$", lines[k + 2]), lines[k + 2]
