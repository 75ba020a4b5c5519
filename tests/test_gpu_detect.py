"""dal3_center_decode + dal3_nms behind 3dal_pytorch_amd/detect.py on the GPU, against what the reference's own
CenterHead.predict / post_processing recorded on tests/nms_ref.py's seeded head maps (tests/golden/nms.npz): the candidate
cells and labels exactly, x / y / z / vel bit for bit, score / dim / rot within the measured bar, the merged ret_list,
the prediction dictionary, the overflow report and the refusals.

BAR_ULPS: score = 1 / (1 + exp(-x)), dim = exp(x) and rot = atan2(s, c) come from the device's libm here and from torch's
vectorised CPU libm in the fixture; both are a few ulps. The worst deviation measured on the MI355X
(profiles/nms_measured.json; every figure is printed before it is asserted) is 2 float32 ulps (score), 1 (dim), 2 (rot);
the bar is twice the worst, and never above 1e-5 relative."""
import importlib
import pickle

import numpy as np
import pytest
import torch

import nms_ref
from _common import golden

hip = importlib.import_module("3dal_pytorch_amd._hip")
detect = importlib.import_module("3dal_pytorch_amd.detect")
track = importlib.import_module("3dal_pytorch_amd.track")
pytestmark = pytest.mark.gpu
DEV = "cuda"
HEAD_RUNS = {"ref_vel": ("ref", True), "ref_novel": ("ref", False), "small_vel": ("small", True), "circle_vel": ("circle", True)}
BAR_ULPS = 4
BAR_REL = 1e-5
NUM_CLASSES = nms_ref.HEAD["num_classes"]
B = nms_ref.HEAD["B"]


def preds(tasks):
    return [{k: torch.from_numpy(v).to(DEV) for k, v in t.items()} for t in tasks]


def post_of(cfg_name, **kw):
    return detect.CenterHeadPost(nms_ref.as_test_cfg(nms_ref.CONFIGS[cfg_name]), NUM_CLASSES, **kw)


def ulps(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)))


def check_boxes(got, want, vel, what):
    """exact columns bit for bit, the libm columns within the bar -> the worst ulps of (dim, rot)"""
    assert got.shape == want.shape, what
    exact = [0, 1, 2] + ([6, 7] if vel else [])
    assert np.array_equal(got[:, exact].view(np.uint32), want[:, exact].view(np.uint32)), what
    u_dim, u_rot = ulps(got[:, 3:6], want[:, 3:6]), ulps(got[:, -1], want[:, -1])
    print(f"{what}: dim {u_dim:.2f} ulps, rot {u_rot:.2f} ulps")
    assert max(u_dim, u_rot) <= BAR_ULPS, what
    np.testing.assert_allclose(got[:, 3:6], want[:, 3:6], rtol=BAR_REL, atol=0)
    np.testing.assert_allclose(got[:, -1], want[:, -1], rtol=BAR_REL, atol=0)
    return u_dim, u_rot


def check_scores(got, want, what):
    u = ulps(got, want)
    print(f"{what}: score {u:.2f} ulps")
    assert u <= BAR_ULPS, what
    np.testing.assert_allclose(got, want, rtol=BAR_REL, atol=0)
    return u


@pytest.mark.parametrize("run", sorted(HEAD_RUNS))
def test_candidates_and_values_against_the_reference(run):
    g = golden("nms")
    cfg_name, vel = HEAD_RUNS[run]
    tasks = nms_ref.head_maps(int(g["head_seed"]), vel)
    r = post_of(cfg_name).decode_nms(preds(tasks))
    assert int(r["status"][0]) == 0
    off, count = r["seg_offsets"], r["seg_count"].cpu().numpy()
    assert r["boxes"].shape[1] == (9 if vel else 7)
    for t in range(len(tasks)):
        for b in range(B):
            f, key = t * B + b, f"head_{run}_t{t}_b{b}_"
            rows = slice(int(off[f]), int(off[f]) + int(count[f]))
            assert count[f] == g[key + "cell"].size > 0, key
            assert np.array_equal(r["cell"][rows].cpu().numpy(), g[key + "cell"]), key
            assert np.array_equal(r["labels"][rows].cpu().numpy(), g[key + "label"]), key
            check_boxes(r["boxes"][rows].cpu().numpy(), g[key + "boxes"], vel, key + "boxes")
            check_scores(r["scores"][rows].cpu().numpy(), g[key + "score"], key + "score")


def _decode_entry(task, cfg, max_workgroups):
    """dal3_center_decode on one task's NCHW maps, every cell a row of capacity -> (cell, labels, boxes, scores, counts)"""
    maps = {k: detect._map(torch.from_numpy(v).to(DEV), "NCHW", None, k) for k, v in task.items()}
    n, H, W, C = maps["hm"].shape
    off = torch.arange(n + 1, dtype=torch.int64, device=DEV) * (H * W)
    K = n * H * W
    boxes, scores = torch.empty((K, 9), dtype=torch.float32, device=DEV), torch.empty(K, dtype=torch.float32, device=DEV)
    labels, cell = torch.empty(K, dtype=torch.int32, device=DEV), torch.empty(K, dtype=torch.int32, device=DEV)
    count, status = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    lib = hip.lib()
    ws = torch.empty(lib.dal3_center_decode_workspace_bytes(n, H, W), dtype=torch.uint8, device=DEV)
    a = hip.CenterDecodeArgs(B=n, H=H, W=W, C=C, has_range=1, out_size_factor=float(cfg["out_size_factor"]),
                             score_threshold=float(cfg["score_threshold"]), F=n, K=K, seg_first=0, seg_step=1,
                             seg_offsets=hip.ptr(off), boxes=hip.ptr(boxes), scores=hip.ptr(scores), labels=hip.ptr(labels),
                             cell=hip.ptr(cell), seg_count=hip.ptr(count), status=hip.ptr(status),
                             max_workgroups=max_workgroups, workspace=hip.ptr(ws), workspace_bytes=ws.numel(),
                             **{k: detect._map_struct(v) for k, v in maps.items()})
    a.voxel_size[:], a.pc_range[:], a.range[:] = cfg["voxel_size"], cfg["pc_range"], cfg["post_center_limit_range"]
    hip.check(lib.dal3_center_decode(a, hip.stream()))
    assert int(status[0]) == 0
    return cell.cpu().numpy(), labels.cpu().numpy(), boxes.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("H,W", [(31, 33), (32, 32), (25, 41)])
def test_rows_and_order_at_the_decode_chunk_edge(H, W):
    """1023, 1024 and 1025 cells: one short of a compaction chunk, the full chunk, one cell in a second chunk. Rows, their
    order, the scores and `cell` against the NumPy restatement, whatever the grid."""
    cfg = dict(nms_ref.CONFIGS["ref"], score_threshold=0.17)     # the better of two classes: a third of the cells above
    (task,) = nms_ref.head_maps(1000 + W, True, B=2, H=H, W=W, num_classes=[2])
    want = nms_ref.decode(task, cfg)
    for wg in (0, 1):
        cell, labels, boxes, scores, count = _decode_entry(task, cfg, wg)
        for b, (w_cell, w_label, w_boxes, w_score) in enumerate(want):
            assert 0.25 * H * W < w_cell.size < 0.42 * H * W        # about a third of the cells survive
            rows = slice(b * H * W, b * H * W + int(count[b]))
            assert count[b] == w_cell.size and np.array_equal(cell[rows], w_cell), (wg, b)
            assert np.array_equal(labels[rows], w_label), (wg, b)
            check_boxes(boxes[rows], w_boxes, True, f"{H}x{W} grid {wg} sample {b} boxes")
            check_scores(scores[rows], w_score, f"{H}x{W} grid {wg} sample {b} score")


def test_nhwc_views_give_the_same_bits():
    g = golden("nms")
    tasks = nms_ref.head_maps(int(g["head_seed"]), True)
    post = post_of("ref")
    a = post.decode_nms(preds(tasks))
    nhwc = [{k: v.permute(0, 2, 3, 1).contiguous() for k, v in t.items()} for t in preds(tasks)]
    b = post.decode_nms(nhwc, layout="NHWC")
    assert torch.equal(a["seg_count"], b["seg_count"]) and torch.equal(a["keep_count"], b["keep_count"])
    off, count = a["seg_offsets"], a["seg_count"].cpu().numpy()
    for f in range(count.size):
        rows = slice(int(off[f]), int(off[f]) + int(count[f]))
        for k in ("boxes", "scores", "labels", "cell"):
            assert a[k][rows].cpu().numpy().tobytes() == b[k][rows].cpu().numpy().tobytes(), (f, k)
        n = int(a["keep_count"][f])
        assert torch.equal(a["keep"][f, :n], b["keep"][f, :n])


@pytest.mark.parametrize("run", sorted(HEAD_RUNS))
def test_predict_returns_the_references_ret_list(run):
    g = golden("nms")
    cfg_name, vel = HEAD_RUNS[run]
    tasks = nms_ref.head_maps(int(g["head_seed"]), vel)
    inputs = preds(tasks)
    before = [{k: v.clone() for k, v in t.items()} for t in inputs]
    meta = [{"token": tok} for tok in nms_ref.TOKENS]
    ret_list = post_of(cfg_name).predict(inputs, metadata=meta)
    assert all(torch.equal(v, before[t][k]) for t, d in enumerate(inputs) for k, v in d.items())   # left as they were
    assert len(ret_list) == B
    for b, ret in enumerate(ret_list):
        assert set(ret) == {"box3d_lidar", "scores", "label_preds", "metadata"} and ret["metadata"] is meta[b]
        assert ret["label_preds"].dtype == torch.int64 and ret["scores"].dtype == torch.float32
        assert ret["box3d_lidar"].is_cuda and ret["box3d_lidar"].dtype == torch.float32
        want_labels = g[f"head_{run}_ret{b}_labels"]
        assert np.array_equal(ret["label_preds"].cpu().numpy(), want_labels)              # order, task offsets
        assert want_labels.max() == sum(NUM_CLASSES) - 1 and want_labels.min() == 0
        check_boxes(ret["box3d_lidar"].cpu().numpy(), g[f"head_{run}_ret{b}_boxes"], vel, f"{run} ret{b} boxes")
        check_scores(ret["scores"].cpu().numpy(), g[f"head_{run}_ret{b}_scores"], f"{run} ret{b} scores")
    none = post_of(cfg_name).predict(inputs)
    assert [r["metadata"] for r in none] == [None] * B


def test_to_prediction_is_what_the_tracking_run_loads(tmp_path):
    g = golden("nms")
    tasks = nms_ref.head_maps(int(g["head_seed"]), True)
    post = post_of("ref")
    ret_list = post.predict(preds(tasks), metadata=[{"token": tok} for tok in nms_ref.TOKENS])
    pred = post.to_prediction(ret_list)
    assert list(pred) == nms_ref.TOKENS
    path = tmp_path / "prediction.pkl"
    with open(path, "wb") as f:
        pickle.dump(pred, f)
    loaded = track._load(str(path))
    frames, tokens = [], list(loaded)
    for tok in [tokens[i] for i in track.sort_order(tokens)]:
        det = loaded[tok]
        assert not det["box3d_lidar"].is_cuda and det["metadata"]["token"] == tok
        frames.append({"frame_id": int(tok.split("_")[3][:-4]), "timestamp": 0.1 * len(frames),
                       "box3d": track._np(det["box3d_lidar"]).astype(np.float32), "label": track._np(det["label_preds"]),
                       "score": track._np(det["scores"]).astype(np.float32), "pose": np.eye(4).reshape(-1)})
    inp = track.TrackInputs(frames)
    assert inp.counts.tolist() == [int(g[f"head_ref_vel_ret{b}_scores"].size) for b in range(B)]
    assert np.array_equal(inp.label, np.concatenate([g[f"head_ref_vel_ret{b}_labels"] for b in range(B)]))


def test_overflow_sets_the_status_bit_and_leaves_the_rows_intact():
    g = golden("nms")
    tasks = nms_ref.head_maps(int(g["head_seed"]), True)
    cap = 10
    post = post_of("ref", capacity=cap)
    r = post.decode_nms(preds(tasks))
    assert int(r["status"][0]) & hip.DECODE_OVERFLOW
    assert r["seg_offsets"].tolist() == [cap * f for f in range(len(tasks) * B + 1)] and r["boxes"].shape[0] == cap * len(tasks) * B
    assert r["seg_count"].cpu().tolist() == [cap] * (len(tasks) * B)
    for t in range(len(tasks)):
        for b in range(B):
            f = t * B + b                       # every segment holds ITS first rows: no neighbour wrote into it
            assert np.array_equal(r["cell"][f * cap:(f + 1) * cap].cpu().numpy(), g[f"head_ref_vel_t{t}_b{b}_cell"][:cap])
            assert np.array_equal(r["labels"][f * cap:(f + 1) * cap].cpu().numpy(), g[f"head_ref_vel_t{t}_b{b}_label"][:cap])
    with pytest.raises(RuntimeError, match="capacity"):
        post.predict(preds(tasks))


def test_refusals():
    cfg = nms_ref.as_test_cfg(nms_ref.CONFIGS["ref"])
    for key in ("double_flip", "per_class_nms"):
        with pytest.raises(ValueError, match=key):
            detect.CenterHeadPost(dict(cfg, **{key: True}), NUM_CLASSES)
    tasks = preds(nms_ref.head_maps(0, True))
    with pytest.raises(ValueError, match="tasks"):
        post_of("ref").decode_nms(tasks[:1])
    with pytest.raises(TypeError, match="float32"):
        post_of("ref").decode_nms([{k: v.double() for k, v in t.items()} for t in tasks])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        post_of("ref").decode_nms([{k: v.cpu() for k, v in t.items()} for t in tasks])
