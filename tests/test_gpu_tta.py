"""The double-flip test-time augmentation on the GPU: dal3_center_decode_flip4 behind detect.DoubleFlipPost,
dal3_flip4_points behind pillars.double_flip, and the detector's route through both.

Against what the reference's own CenterHead.predict with double_flip recorded on tests/tta_ref.py's seeded maps
(tests/golden/tta.npz: four independent random views per sample on a 12 x 20 grid): the merged samples' candidate cells
and labels exactly, x / y / z / vel bit for bit (sums of four and one division in torch's order), score / dim / rot within
the bar; the merged ret_list. Against the NumPy restatement: the compaction's chunk edge, degenerate and self-mirrored
grids. By construction: views rebuilt from one view give that view's plain decode back bit for bit; every layout gives
the same bytes; an overflowing segment keeps its own first rows. The flipped points bitwise, and `detect` / `forward`
against the stages composed by hand.

BAR_ULPS: score is a mean of four 1 / (1 + exp(-x)), dim a mean of four exp(x), from the device's libm here and from
torch's vectorised CPU libm in the fixture, each a few ulps apart; rot = atan2 of means that are bit-exact. The worst
deviation measured on the MI355X against the fixture (profiles/tta_measured.json; every figure is printed before it is
asserted) is 2 float32 ulps (score), 2 (dim), 2 (rot); the bar is twice the worst, and never above 1e-5
relative: tests/test_gpu_detect.py's rule. DAL3_TTA_RECORD=<path> writes the figures this file measured."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import nms_ref
import pillars_ref as P
import rpn_ref as R
import tta_ref
from _common import golden

hip = importlib.import_module("3dal_pytorch_amd._hip")
detect = importlib.import_module("3dal_pytorch_amd.detect")
pillars = importlib.import_module("3dal_pytorch_amd.pillars")
detector = importlib.import_module("3dal_pytorch_amd.detector")
pytestmark = pytest.mark.gpu
DEV = "cuda"
MEASURED = {"score": 2.0, "dim": 2.0, "rot": 2.0}          # worst ulps against the fixture (profiles/tta_measured.json)
BAR_ULPS = 2 * max(MEASURED.values())
BAR_REL = 1e-5
NUM_CLASSES = tta_ref.HEAD["num_classes"]
B = tta_ref.HEAD["B"] // 4                                  # merged samples of the fixture
_RECORD = {}                                                # column -> worst ulps against the FIXTURE


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    path = os.environ.get("DAL3_TTA_RECORD")
    if path and _RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


def preds(tasks):
    return [{k: torch.from_numpy(v).to(DEV) for k, v in t.items()} for t in tasks]


def flip_cfg(cfg_name, **kw):
    return dict(nms_ref.as_test_cfg(dict(nms_ref.CONFIGS[cfg_name], **kw)), double_flip=True)


def post_of(cfg_name, **kw):
    return detect.DoubleFlipPost(flip_cfg(cfg_name), NUM_CLASSES, **kw)


def ulps(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)))


def check_boxes(got, want, vel, what, record=False):
    """exact columns bit for bit, the libm columns within the bar"""
    assert got.shape == want.shape, what
    exact = [0, 1, 2] + ([6, 7] if vel else [])
    assert np.array_equal(got[:, exact].view(np.uint32), want[:, exact].view(np.uint32)), what
    u_dim, u_rot = ulps(got[:, 3:6], want[:, 3:6]), ulps(got[:, -1], want[:, -1])
    print(f"{what}: dim {u_dim:.2f} ulps, rot {u_rot:.2f} ulps")
    if record:
        _RECORD["dim"], _RECORD["rot"] = max(_RECORD.get("dim", 0.0), u_dim), max(_RECORD.get("rot", 0.0), u_rot)
    assert max(u_dim, u_rot) <= BAR_ULPS, what
    np.testing.assert_allclose(got[:, 3:6], want[:, 3:6], rtol=BAR_REL, atol=0)
    np.testing.assert_allclose(got[:, -1], want[:, -1], rtol=BAR_REL, atol=0)


def check_scores(got, want, what, record=False):
    u = ulps(got, want)
    print(f"{what}: score {u:.2f} ulps")
    if record:
        _RECORD["score"] = max(_RECORD.get("score", 0.0), u)
    assert u <= BAR_ULPS, what
    np.testing.assert_allclose(got, want, rtol=BAR_REL, atol=0)


def rows_of(r, f):
    off, count = r["seg_offsets"], r["seg_count"].cpu().numpy()
    return slice(int(off[f]), int(off[f]) + int(count[f]))


# ------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("run", sorted(tta_ref.RUNS))
def test_merged_candidates_and_values_against_the_reference(run):
    g = golden("tta")
    cfg_name, vel = tta_ref.RUNS[run]
    tasks = tta_ref.head_maps(int(g["tta_seed"]), vel)
    r = post_of(cfg_name).decode_nms(preds(tasks))
    assert int(r["status"][0]) == 0 and r["B"] == B and r["seg_count"].numel() == len(tasks) * B
    assert r["boxes"].shape[1] == (9 if vel else 7)
    count = r["seg_count"].cpu().numpy()
    for t in range(len(tasks)):
        for b in range(B):
            f, key = t * B + b, f"tta_{run}_t{t}_b{b}_"
            rows = rows_of(r, f)
            assert count[f] == g[key + "cell"].size > 0, key
            assert np.array_equal(r["cell"][rows].cpu().numpy(), g[key + "cell"]), key
            assert np.array_equal(r["labels"][rows].cpu().numpy(), g[key + "label"]), key
            check_boxes(r["boxes"][rows].cpu().numpy(), g[key + "boxes"], vel, key + "boxes", record=True)
            check_scores(r["scores"][rows].cpu().numpy(), g[key + "score"], key + "score", record=True)


@pytest.mark.parametrize("run", sorted(tta_ref.RUNS))
def test_predict_returns_the_references_merged_ret_list(run):
    g = golden("tta")
    cfg_name, vel = tta_ref.RUNS[run]
    inputs = preds(tta_ref.head_maps(int(g["tta_seed"]), vel))
    before = [{k: v.clone() for k, v in t.items()} for t in inputs]
    meta = [{"token": tok} for tok in tta_ref.TOKENS]
    post = post_of(cfg_name)
    ret_list = post.predict(inputs, metadata=meta)
    assert all(torch.equal(v, before[t][k]) for t, d in enumerate(inputs) for k, v in d.items())   # left as they were
    assert len(ret_list) == B
    for b, ret in enumerate(ret_list):
        assert set(ret) == {"box3d_lidar", "scores", "label_preds", "metadata"}
        assert ret["metadata"] is meta[4 * b]                       # every fourth: the unflipped view's
        assert ret["label_preds"].dtype == torch.int64 and ret["box3d_lidar"].is_cuda
        want_labels = g[f"tta_{run}_ret{b}_labels"]
        assert np.array_equal(ret["label_preds"].cpu().numpy(), want_labels)              # order, task offsets
        assert want_labels.max() == sum(NUM_CLASSES) - 1 and want_labels.min() == 0
        check_boxes(ret["box3d_lidar"].cpu().numpy(), g[f"tta_{run}_ret{b}_boxes"], vel, f"{run} ret{b} boxes", record=True)
        check_scores(ret["scores"].cpu().numpy(), g[f"tta_{run}_ret{b}_scores"], f"{run} ret{b} scores", record=True)
    two = post.predict(inputs, metadata=meta[::4])                  # one entry per merged sample
    assert [r["metadata"] for r in two] == meta[::4] and torch.equal(two[1]["scores"], ret_list[1]["scores"])
    assert [r["metadata"] for r in post.predict(inputs)] == [None] * B
    pred = post.to_prediction(ret_list)
    assert list(pred) == [tta_ref.TOKENS[0], tta_ref.TOKENS[4]]


# ------------------------------------------------------------------------------- 2 - 4. the entry itself
def _entry(task, cfg, max_workgroups, flip):
    """dal3_center_decode_flip4 (or dal3_center_decode) on one task's NCHW maps, every cell a row of capacity -> (cell,
    labels, boxes, scores, counts)"""
    maps = {k: detect._map(torch.from_numpy(np.ascontiguousarray(v)).to(DEV), "NCHW", None, k) for k, v in task.items()}
    n_maps, H, W, C = maps["hm"].shape
    n = n_maps // 4 if flip else n_maps
    off = torch.arange(n + 1, dtype=torch.int64, device=DEV) * (H * W)
    K = n * H * W
    boxes, scores = torch.empty((K, 9), dtype=torch.float32, device=DEV), torch.empty(K, dtype=torch.float32, device=DEV)
    labels, cell = torch.empty(K, dtype=torch.int32, device=DEV), torch.empty(K, dtype=torch.int32, device=DEV)
    count, status = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    lib = hip.lib()
    nbytes = (lib.dal3_center_decode_flip4_workspace_bytes if flip else lib.dal3_center_decode_workspace_bytes)(n, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    a = hip.CenterDecodeArgs(B=n, H=H, W=W, C=C, has_range=1, out_size_factor=float(cfg["out_size_factor"]),
                             score_threshold=float(cfg["score_threshold"]), F=n, K=K, seg_first=0, seg_step=1,
                             seg_offsets=hip.ptr(off), boxes=hip.ptr(boxes), scores=hip.ptr(scores), labels=hip.ptr(labels),
                             cell=hip.ptr(cell), seg_count=hip.ptr(count), status=hip.ptr(status),
                             max_workgroups=max_workgroups, workspace=hip.ptr(ws), workspace_bytes=ws.numel(),
                             **{k: detect._map_struct(v) for k, v in maps.items()})
    a.voxel_size[:], a.pc_range[:], a.range[:] = cfg["voxel_size"], cfg["pc_range"], cfg["post_center_limit_range"]
    if flip:
        hip.check(lib.dal3_center_decode_flip4(hip.CenterDecodeFlip4Args(decode=a), hip.stream()))
    else:
        hip.check(lib.dal3_center_decode(a, hip.stream()))
    assert int(status[0]) == 0
    return cell.cpu().numpy(), labels.cpu().numpy(), boxes.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy()


def _against_the_restatement(task, cfg, H, W, grids, lo, hi):
    want = tta_ref.merge_decode(task, cfg)
    for wg in grids:
        cell, labels, boxes, scores, count = _entry(task, cfg, wg, True)
        assert count.size == len(want)
        for b, (w_cell, w_label, w_boxes, w_score) in enumerate(want):
            assert lo <= w_cell.size <= hi, (b, w_cell.size)
            rows = slice(b * H * W, b * H * W + int(count[b]))
            assert count[b] == w_cell.size and np.array_equal(cell[rows], w_cell), (wg, b)
            assert np.array_equal(labels[rows], w_label), (wg, b)
            check_boxes(boxes[rows], w_boxes, True, f"{H}x{W} grid {wg} sample {b} boxes")
            check_scores(scores[rows], w_score, f"{H}x{W} grid {wg} sample {b} score")


@pytest.mark.parametrize("H,W", [(31, 33), (32, 32), (25, 41)])
def test_rows_and_order_at_the_decode_chunk_edge(H, W):
    """1023, 1024 and 1025 cells: one short of a compaction chunk, the full chunk, one cell in a second chunk; two merged
    samples (8 maps), two classes. Rows, their order, the values and `cell` against the restatement, whatever the grid.
    The better of two classes' mean of four sigmoids is above 0.17 in about 27 % of the cells."""
    cfg = dict(nms_ref.CONFIGS["ref"], score_threshold=0.17)
    (task,) = nms_ref.head_maps(2000 + W, True, B=8, H=H, W=W, num_classes=[2])
    _against_the_restatement(task, cfg, H, W, (0, 1), 0.2 * H * W, 0.4 * H * W)


@pytest.mark.parametrize("H,W", [(1, 7), (5, 1), (3, 3)])
def test_degenerate_and_self_mirrored_grids(H, W):
    """one row, one column, and odd sizes whose middle row and column are their own mirror images; one merged sample"""
    cfg = nms_ref.CONFIGS["ref"]
    (task,) = nms_ref.head_maps(3000 + W, True, B=4, H=H, W=W, num_classes=[2])
    _against_the_restatement(task, cfg, H, W, (0, 1), 1, H * W)


def test_views_rebuilt_from_one_view_give_its_plain_decode_back_bit_for_bit():
    """views 1-3 are view 0 under the inverse transform, reg a multiple of 2^-10 so that 1 - reg is exact: every merged
    value is a mean of four equal float32 values, which is that value — the libm columns included"""
    cfg = nms_ref.CONFIGS["ref"]
    H, W = 13, 21
    (one,) = nms_ref.head_maps(4000, True, B=2, H=H, W=W, num_classes=[2])
    one["reg"] = (np.round(one["reg"] * 1024) / 1024).astype(np.float32)
    assert np.array_equal((np.float32(1) - (np.float32(1) - one["reg"])), one["reg"])
    plain = _entry(one, cfg, 0, False)
    merged = _entry(tta_ref.mirrored_views(one), cfg, 0, True)
    assert plain[4].tolist() == merged[4].tolist() and all(0.25 * H * W < n < H * W for n in plain[4])
    for b in range(2):
        rows = slice(b * H * W, b * H * W + int(plain[4][b]))
        for k, name in enumerate(("cell", "labels", "boxes", "scores")):
            assert plain[k][rows].tobytes() == merged[k][rows].tobytes(), (b, name)


# ------------------------------------------------------------------------------- 5, 6. layouts, overflow
def test_every_layout_gives_the_same_bytes():
    g = golden("tta")
    nchw = preds(tta_ref.head_maps(int(g["tta_seed"]), True))
    post = post_of("ref")
    a = post.decode(nchw)
    nhwc = [{k: v.permute(0, 2, 3, 1).contiguous() for k, v in t.items()} for t in nchw]
    keys = ("reg", "height", "dim", "rot", "vel", "hm")
    sliced = []
    for t in nchw:                              # channel slices of one wider tensor per task: what the head hands over
        wide = torch.cat([t[k] for k in keys], 1)
        at, d = 0, {}
        for k in keys:
            d[k] = wide[:, at:at + t[k].shape[1]]
            at += t[k].shape[1]
        assert not d["hm"].is_contiguous()
        sliced.append(d)
    for what, b in (("NHWC", post.decode(nhwc, layout="NHWC")), ("slices", post.decode(sliced))):
        assert torch.equal(a["seg_count"], b["seg_count"]) and int(b["status"][0]) == 0
        for f in range(a["seg_count"].numel()):
            rows = rows_of(a, f)
            assert rows.stop > rows.start
            for k in ("boxes", "scores", "labels", "cell"):
                assert a[k][rows].cpu().numpy().tobytes() == b[k][rows].cpu().numpy().tobytes(), (what, f, k)


def test_overflow_sets_the_status_bit_and_leaves_the_rows_intact():
    g = golden("tta")
    tasks = tta_ref.head_maps(int(g["tta_seed"]), True)
    cap = 10
    post = post_of("ref", capacity=cap)
    r = post.decode_nms(preds(tasks))
    assert int(r["status"][0]) & hip.DECODE_OVERFLOW
    assert r["seg_offsets"].tolist() == [cap * f for f in range(len(tasks) * B + 1)] and r["boxes"].shape[0] == cap * len(tasks) * B
    assert r["seg_count"].cpu().tolist() == [cap] * (len(tasks) * B)
    for t in range(len(tasks)):
        for b in range(B):
            f = t * B + b                       # every segment holds ITS first rows: no neighbour wrote into it
            assert np.array_equal(r["cell"][f * cap:(f + 1) * cap].cpu().numpy(), g[f"tta_ref_vel_t{t}_b{b}_cell"][:cap])
            assert np.array_equal(r["labels"][f * cap:(f + 1) * cap].cpu().numpy(), g[f"tta_ref_vel_t{t}_b{b}_label"][:cap])
    with pytest.raises(RuntimeError, match="capacity"):
        post.predict(preds(tasks))


# ------------------------------------------------------------------------------- 7. the points
def _points(n, C, seed):
    pts = np.random.default_rng(seed).normal(0, 30, (n, C)).astype(np.float32)
    if n >= 8:
        special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf], np.float32)
        pts[:5, 0], pts[2:7, 1] = special, special
        pts[7, :2] = np.array([0x7fc12345, 0xffc00001], np.uint32).view(np.float32)      # NaNs with a payload, either sign
    return pts


@pytest.mark.parametrize("C,offsets", [(2, [0, 300]), (5, [0, 1000, 1000, 1531]), (6, [0, 257, 700]), (5, [0, 0]), (5, [0, 9])])
def test_flipped_points_bitwise_against_the_restatement(C, offsets):
    """C = 2 (nothing but x, y), 5, 6; three samples with an empty one; no point at all; row counts that are no multiple
    of the 256-thread block; 0.0, -0.0, NaN (payload kept) and inf in the negated columns. Every byte of out and the
    offsets, for a free grid and for one workgroup."""
    n = offsets[-1]
    pts = _points(n, C, 50 + C + n)
    want, want_off = tta_ref.flip4_points(pts, offsets)
    for wg in (0, 1):
        out, off, off_dev = pillars.double_flip(torch.from_numpy(pts).to(DEV), offsets, max_workgroups=wg)
        assert out.shape == (4 * n, C) and off.dtype == np.int64 and off_dev.dtype == torch.int64
        assert off.tolist() == want_off.tolist() == off_dev.cpu().tolist()
        assert out.cpu().numpy().view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), wg
    if n >= 8:
        got = out.cpu().numpy().view(np.uint32)
        first = pts.view(np.uint32)
        n0 = offsets[1]
        assert np.array_equal(got[n0:n0 + 8, 1], first[:8, 1] ^ 0x80000000) and np.array_equal(got[n0:n0 + 8, 0], first[:8, 0])
        assert np.array_equal(got[2 * n0:2 * n0 + 8, 0], first[:8, 0] ^ 0x80000000)


def test_flipped_points_take_device_offsets_and_enqueue_without_a_synchronisation():
    pts = torch.from_numpy(_points(700, 5, 9)).to(DEV)
    offsets = [0, 257, 700]
    off_dev = torch.tensor(offsets, dtype=torch.int64, device=DEV)
    want, want_off = tta_ref.flip4_points(pts.cpu().numpy(), offsets)
    hip.lib()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, off, out_dev = pillars.double_flip(pts, offsets, off_dev)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out.cpu().numpy().view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    assert out_dev.cpu().tolist() == want_off.tolist() == off.tolist()


# ------------------------------------------------------------------------------- 8. the detector
# tests/test_gpu_detector.py's tiny model: a 44 x 36 grid of pillars, one task of three classes
VOXEL, RANGE = (0.32, 0.32, 6.0), (0.0, -5.76, -2.0, 14.08, 5.76, 4.0)
COUNTS = (3000, 1900)
TEST_CFG = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0],
                nms=dict(nms_pre_max_size=1000, nms_post_max_size=83, nms_iou_threshold=0.2), score_threshold=0.3,
                pc_range=[RANGE[0], RANGE[1]], out_size_factor=1, voxel_size=[0.32, 0.32])
FLIP_CFG = dict(TEST_CFG, double_flip=True)
MODEL = dict(reader=dict(type="PillarFeatureNet", num_filters=[64, 64], num_input_features=5, with_distance=False,
                         voxel_size=VOXEL, pc_range=RANGE),
             backbone=dict(type="PointPillarsScatter", ds_factor=1), neck=dict(type="RPN", **R.NECK),
             bbox_head=dict(type="CenterHead", **R.HEAD))
META = [{"token": "seq0_frame7", "num_point_features": 5}, {"token": "seq0_frame8", "num_point_features": 5}]


def sweep():
    n = sum(COUNTS)
    lo, hi = np.asarray(RANGE[:3]), np.asarray(RANGE[3:])
    xyz = P.synth.uniform(R.SEED, "sweep/xyz", (n, 3)) * (hi - lo) * 1.04 + lo - 0.02 * (hi - lo)       # a few fall outside
    pts = np.concatenate([xyz, P.synth.uniform(R.SEED, "sweep/f", (n, 2))], 1).astype(np.float32)
    return pts, np.asarray([0, COUNTS[0], n], np.int64)


@pytest.fixture(scope="module")
def model():
    sd = {"reader." + k: v for k, v in P.reader_weights(2, 5).items()}
    sd.update({"neck." + k: v for k, v in R.neck_weights().items()})
    sd.update({"bbox_head." + k: v for k, v in R.head_weights().items()})
    m = detector.PointPillars(**MODEL, test_cfg=FLIP_CFG, max_points=20, max_voxels=2000)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.cuda().eval()


def _same(a, b, n=2):
    assert len(a) == len(b) == n
    for x, y in zip(a, b):
        assert set(x) == set(y) == {"box3d_lidar", "scores", "label_preds", "metadata"}
        for k in ("box3d_lidar", "scores", "label_preds"):
            assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), k
        assert x["metadata"] is y["metadata"]


def _dense(model, r, n):
    canvas = model.reader.forward_canvas(r.voxels, r.num_points, r.coordinates, n, [44, 36], n_pillars=r.n_pillars)
    assert canvas.shape == (n, 64, 36, 44)
    with torch.no_grad():
        return model.bbox_head(model.neck(canvas))


def test_detect_and_forward_with_double_flip_equal_the_stages_composed_by_hand(model):
    pts, off = sweep()
    dpts = torch.from_numpy(pts).to(DEV)
    # ---- by hand
    flipped, off4, off4_dev = pillars.double_flip(dpts, off)
    r = pillars.voxelize(flipped, off4, VOXEL, RANGE, 20, 2000, point_offsets_device=off4_dev)
    preds8 = _dense(model, r, 8)
    want = detect.DoubleFlipPost(FLIP_CFG, [3]).predict(preds8, metadata=META)
    n = [int(w["scores"].numel()) for w in want]
    assert all(0 < k <= 83 for k in n), n
    plain_of_view0 = detect.CenterHeadPost(TEST_CFG, [3]).predict([{k: v[0::4] for k, v in preds8[0].items()}])
    assert not all(torch.equal(a["scores"], b["scores"]) for a, b in zip(want, plain_of_view0))   # the merge changes the result
    # ---- detect(points, offsets): B metadata entries, `last` is the 4 B samples' voxelisation of the restated flipped points
    model.test_cfg = FLIP_CFG
    got = model.detect(dpts, off, metadata=META)
    _same(got, want)
    ref_pts, ref_off = tta_ref.flip4_points(pts, off)
    assert ref_off.tolist() == off4.tolist()
    rr = pillars.voxelize(torch.from_numpy(ref_pts).to(DEV), ref_off, VOXEL, RANGE, 20, 2000)
    assert model.last.B == 8 and torch.equal(model.last.voxel_offsets, rr.voxel_offsets)
    m = int(rr.voxel_offsets[-1])
    counts = (rr.voxel_offsets[1:] - rr.voxel_offsets[:-1]).cpu().tolist()
    assert counts[0] > 0 and counts[1] > 0 and counts[4] > 0 and counts[5] > 0, counts      # the views that stay in the range
    for k in ("voxels", "coordinates", "num_points"):
        assert torch.equal(getattr(model.last, k)[:m], getattr(rr, k)[:m]), k
    assert list(model.to_prediction(got)) == ["seq0_frame7", "seq0_frame8"]
    _same(model.detect(dpts, off, metadata=META, point_offsets_device=torch.from_numpy(off).to(DEV)), want)
    # ---- forward(example): the reference's collated batch of 4 B samples, every view with its sample's metadata
    voxels, coords, num, nv = r.finish()
    meta8 = [META[i // 4] for i in range(8)]
    example = dict(voxels=voxels, coordinates=coords, num_points=num, num_voxels=nv, shape=[[44, 36, 1]] * 8, metadata=meta8)
    with torch.no_grad():
        _same(model(example, return_loss=False), want)
    # ---- without double_flip the route is the plain one
    model.test_cfg = TEST_CFG
    try:
        r2 = pillars.voxelize(dpts, off, VOXEL, RANGE, 20, 2000)
        plain = detect.CenterHeadPost(TEST_CFG, [3]).predict(_dense(model, r2, 2), metadata=META)
        _same(model.detect(dpts, off, metadata=META), plain)
        assert model.last.B == 2
        assert isinstance(model.bbox_head._post[1], detect.CenterHeadPost) and model.bbox_head._post[1].VIEWS == 1
    finally:
        model.test_cfg = FLIP_CFG
