"""dal3_score_tracks / dal3_best_gt_iou on the GPU (3dal_pytorch_amd/baseline.py) against what the reference's
tools/static_init.py, tools/dynamic_init.py and tools/eval.py recorded on the seeded work dir of tests/baseline_ref.py
(tests/golden/baseline.npz), against the package's own IoU entries bit for bit, and for the reproducibility of the sums."""
import importlib
import pickle

import numpy as np
import pytest
import torch

import baseline_ref
import iou_ref
from _common import golden
from test_gpu_iou import near_pairs

baseline = importlib.import_module("3dal_pytorch_amd.baseline")
ev = importlib.import_module("3dal_pytorch_amd.eval")
iou = importlib.import_module("3dal_pytorch_amd.iou")
pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5                      # the bound tests/test_gpu_iou.py holds the IoU kernels to against iou_ref
ATOL_BOX = 1e-9                 # the bound tests/test_iou_cpu.py holds eval.metric_samples' boxes to


def bits(t):
    return t.cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint64)


def by_type(types, v3, scored):
    """(pass count, [type 1, 2, 4, other] counts) of the scored samples from per-sample float32 IoUs, in NumPy"""
    t = types[scored]
    thr = np.where(t == 1, np.float32(0.7), np.float32(0.5))
    return int(np.sum(v3[scored] >= thr)), [int(np.sum(t == 1)), int(np.sum(t == 2)), int(np.sum(t == 4)),
                                            int(np.sum(~np.isin(t, [1, 2, 4])))]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    g = golden("baseline")
    paths, c = baseline_ref.write_work_dir(str(tmp_path_factory.mktemp("baseline")), int(g["seed"]))
    with open(paths["infos"], "rb") as f:
        annos = ev.Annos(ev.reorganize_info(pickle.load(f)))
    flats = {}
    for key in ("static", "dynamic"):
        with open(paths[key], "rb") as f:
            track = pickle.load(f)
        flats[key] = baseline.flatten(ev.preprocessing(track, annos) if key == "static" else track, annos)
    return g, flats


@pytest.mark.parametrize("name", baseline_ref.FLAVOURS)
def test_score_tracks_reproduces_the_reference(work, name):
    g, flats = work
    flat = flats["dynamic" if name == "dynamic_init" else "static"]
    rows = flat["best_row"] if name == "static_best" else flat["own_row"]
    scored = flat["has_gt"].astype(bool)
    acc = baseline.ScoreAccumulator(DEV)
    vb, v3, pb, lb = baseline.score_tracks(flat["boxes"], rows, flat["frame"], flat["pose_inv"], flat["gt"], flat["has_gt"],
                                           flat["types"], acc=acc, return_boxes=True, device=DEV)
    # the two boxes the reference hands to its geometry
    pred, label = pb.cpu().numpy(), lb.cpu().numpy()
    print(f"{name}: max |pred - ref| {np.abs(pred[scored] - g[f'{name}_pred']).max():.3e}, "
          f"max |label - ref| {np.abs(label[scored] - g[f'{name}_label']).max():.3e}")
    np.testing.assert_allclose(pred[scored], g[f"{name}_pred"], rtol=0, atol=ATOL_BOX)
    np.testing.assert_allclose(label[scored], g[f"{name}_label"], rtol=0, atol=ATOL_BOX)
    assert np.all(pred[scored, 6] == 0.0)
    assert np.isnan(pred[~scored]).all() and np.isnan(label[~scored]).all()
    # the IoU: the bits of paired_iou on those boxes, and the oracle's value on the recorded ones
    wb, w3 = iou.paired_iou(pb[torch.from_numpy(scored).to(DEV)], lb[torch.from_numpy(scored).to(DEV)])
    got_b, got_3 = vb.cpu().numpy(), v3.cpu().numpy()
    assert np.array_equal(bits(vb)[scored], bits(wb)) and np.array_equal(bits(v3)[scored], bits(w3))
    assert np.isnan(got_b[~scored]).all() and np.isnan(got_3[~scored]).all()
    print(f"{name}: max |iou - oracle| bev {np.abs(got_b[scored] - g[f'{name}_iou_bev']).max():.3e}, "
          f"3d {np.abs(got_3[scored] - g[f'{name}_iou_3d']).max():.3e}")
    assert np.abs(got_b[scored] - g[f"{name}_iou_bev"]).max() <= TOL
    assert np.abs(got_3[scored] - g[f"{name}_iou_3d"]).max() <= TOL
    # the same bits without the optional box outputs
    vb2, v32 = baseline.score_tracks(flat["boxes"], rows, flat["frame"], flat["pose_inv"], flat["gt"], flat["has_gt"],
                                     flat["types"], device=DEV)
    assert np.array_equal(bits(vb2), bits(vb)) and np.array_equal(bits(v32), bits(v3))
    # counts exactly, sums = float64 sums of the kernel's own float32 values
    c = acc.counts()
    assert c["n_iou_3d_pass"] == int(g[f"{name}_n_pass"])
    assert [c["n_type1"], c["n_type2"], c["n_type4"], c["n_other_type"]] == list(g[f"{name}_n_type"])
    assert c["n_scored"] == int(scored.sum()) and c["n_samples"] == int(g[f"{name}_n_samples"]) == len(scored)
    np.testing.assert_allclose(c["sum_iou_bev"], np.sum(got_b[scored], dtype=np.float64), rtol=1e-12, atol=0)
    np.testing.assert_allclose(c["sum_iou_3d"], np.sum(got_3[scored], dtype=np.float64), rtol=1e-12, atol=0)
    r = acc.result()
    assert [f"{r['iou2d']:.4f}", f"{r['iou3d']:.4f}", f"{r['acc']:.4f}"] == [f"{x:.4f}" for x in g[f"{name}_means"]]


def test_sums_are_reproducible_and_accumulate():
    S = 300_000
    a, b = near_pairs(S, 11)
    t = baseline_ref.synthetic_tables(a, b, 12)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in t.items()}

    def run(lo, hi, acc, **kw):
        return baseline.score_tracks(d["boxes"], d["box_row"][lo:hi], d["frame"][lo:hi], d["pose_inv"], d["gt"][lo:hi],
                                     d["has_gt"][lo:hi], d["type"][lo:hi], acc=acc, **kw)
    accs = [baseline.ScoreAccumulator(DEV) for _ in range(4)]
    out = [run(0, S, accs[0]), run(0, S, accs[1]), run(0, S, accs[2], max_workgroups=7)]
    torch.cuda.synchronize()
    words = [x.acc.cpu().numpy().tobytes() for x in accs[:3]]
    assert words[0] == words[1] == words[2]                              # run to run, and whatever the grid
    for o in out[1:]:
        assert np.array_equal(bits(o[0]), bits(out[0][0])) and np.array_equal(bits(o[1]), bits(out[0][1]))
    # the accumulator is what NumPy makes of the kernel's own per-sample values
    vb, v3 = out[0][0].cpu().numpy(), out[0][1].cpu().numpy()
    scored = t["has_gt"].astype(bool)
    assert np.isnan(v3[~scored]).all() and not np.isnan(v3[scored]).any()
    c = accs[0].counts()
    n_pass, n_type = by_type(t["type"], v3, scored)
    assert c["n_iou_3d_pass"] == n_pass and [c["n_type1"], c["n_type2"], c["n_type4"], c["n_other_type"]] == n_type
    assert min(n_type) > 1000 and 1000 < n_pass < scored.sum() - 1000          # both outcomes, every type
    assert c["n_scored"] == int(scored.sum()) and c["n_samples"] == S
    np.testing.assert_allclose(c["sum_iou_bev"], np.sum(vb[scored], dtype=np.float64), rtol=1e-12, atol=0)
    np.testing.assert_allclose(c["sum_iou_3d"], np.sum(v3[scored], dtype=np.float64), rtol=1e-12, atol=0)
    # a sample of the pairs against the oracle, through the restated recipe
    pick = np.nonzero(scored)[0][:2000]
    pred, label = [], []
    for s in pick:
        init = baseline_ref.transform_box(t["boxes"][s][np.newaxis], t["pose_inv"][t["frame"][s]].reshape(4, 4))[0]
        pred.append(np.concatenate([init[:3], baseline_ref.size_round_trip(init[3:6]), [0.0]]))
        label.append(np.concatenate([t["gt"][s, :3].astype(np.float64), baseline_ref.size_round_trip(t["gt"][s, 3:6]),
                                     [baseline_ref.angle_round_trip(t["gt"][s, 6] - init[6])]]))
    want_b, want_3 = iou_ref.paired(np.array(pred), np.array(label))
    assert np.abs(vb[pick] - want_b).max() <= TOL and np.abs(v3[pick] - want_3).max() <= TOL
    # two calls into one accumulator = one call over the concatenation (the split is not a multiple of a chunk)
    cut = 123_457
    run(0, cut, accs[3])
    run(cut, S, accs[3])
    c2 = accs[3].counts()
    for k in c:
        if k.startswith("n_"):
            assert c2[k] == c[k], k
    np.testing.assert_allclose(c2["sum_iou_bev"], c["sum_iou_bev"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(c2["sum_iou_3d"], c["sum_iou_3d"], rtol=1e-12, atol=0)
    # float64 ground truth of the same values: the same bits
    o64 = baseline.score_tracks(d["boxes"], d["box_row"], d["frame"], d["pose_inv"], d["gt"].double(), d["has_gt"], d["type"])
    assert np.array_equal(bits(o64[1]), bits(out[0][1]))
    # a row or a frame outside its table is not scored
    bad_row = d["box_row"][:512].clone()
    bad_row[5], bad_row[300] = S, -1
    o = baseline.score_tracks(d["boxes"], bad_row, d["frame"][:512], d["pose_inv"], d["gt"][:512],
                              torch.ones(512, dtype=torch.uint8, device=DEV), d["type"][:512])
    assert torch.isnan(o[1][[5, 300]]).all() and int(torch.isnan(o[1]).sum()) == 2


def _best_by_numpy(queries, offsets, gts, frame):
    """per query: the maximum of iou.boxes_iou3d over its frame's GT boxes and np.argmax's first index"""
    v, idx = [], []
    for q in range(queries.shape[0]):
        lo, hi = int(offsets[frame[q]]), int(offsets[frame[q] + 1])
        if lo == hi:
            v.append(np.float32("nan"))
            idx.append(-1)
            continue
        row = iou.boxes_iou3d(queries[q:q + 1], gts[lo:hi]).cpu().numpy()[0]
        v.append(np.max(row))
        idx.append(int(np.argmax(row)))
    return np.array(v, np.float32), np.array(idx, np.int32)


def test_best_gt_iou_on_the_label_entries():
    g = golden("baseline")
    Q = len(g["lab_ids"])
    queries = torch.from_numpy(np.concatenate([g["lab_query_track"], g["lab_query_static"]])).to(DEV)
    gts = torch.from_numpy(g["lab_gt"]).to(DEV)
    frame = np.concatenate([np.arange(Q), np.arange(Q)]).astype(np.int32)
    v3, vb, idx = baseline.best_gt_iou(queries, torch.from_numpy(g["lab_gt_offsets"]), gts, torch.from_numpy(frame))
    want, want_idx = _best_by_numpy(queries, g["lab_gt_offsets"], gts, frame)
    assert np.array_equal(bits(v3), want.view(np.uint32)) and np.array_equal(idx.cpu().numpy(), want_idx)
    ref = np.concatenate([g["lab_iou_track"], g["lab_iou_static"]])
    print(f"labels: max |iou - oracle| {np.abs(v3.cpu().numpy() - ref).max():.3e}")
    assert np.abs(v3.cpu().numpy() - ref).max() <= TOL
    n_gt = np.diff(g["lab_gt_offsets"])
    assert n_gt.min() == 1 and n_gt.max() >= 20
    # the BEV IoU is that of the winning pair
    for q in (0, Q - 1, Q):
        lo = int(g["lab_gt_offsets"][frame[q]])
        wb = iou.boxes_iou_bev(queries[q:q + 1], gts[lo + want_idx[q]:lo + want_idx[q] + 1])
        assert bits(vb)[q] == bits(wb)[0, 0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_best_gt_iou_on_a_ragged_set_with_empty_frames_and_ties(dtype):
    rng = np.random.default_rng(21)
    F, Q = 60, 700
    counts = rng.integers(0, 150, F)
    counts[[3, 17, 59]] = 0
    counts[5], counts[6] = 1, 64
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    a, _ = near_pairs(int(offsets[-1]), 22)
    a[:, :2] = rng.uniform(-20, 20, (len(a), 2))                       # crowded: several GT boxes overlap a query
    frame = rng.integers(0, F, Q).astype(np.int32)
    frame[:3] = [3, 17, 59]
    queries = np.zeros((Q, 7))
    dup = 0
    for q in range(Q):
        lo, hi = offsets[frame[q]], offsets[frame[q] + 1]
        if hi > lo:
            k = int(rng.integers(lo, hi))
            queries[q] = a[k] + rng.normal(0, 0.1, 7) * [1, 1, 0.2, 0.3, 0.2, 0.2, 0.3]
            if q % 5 == 0 and hi - lo > 1:                             # an exact tie: the best GT box twice in the range
                other = lo + (k - lo + 1 + int(rng.integers(0, hi - lo - 1))) % (hi - lo)
                a[other] = a[k]
                dup += 1
    assert dup > 50
    qd, gd = torch.from_numpy(queries).to(DEV, dtype), torch.from_numpy(a).to(DEV, dtype)
    v3, vb, idx = baseline.best_gt_iou(qd, torch.from_numpy(offsets), gd, torch.from_numpy(frame))
    v3b, _, idxb = baseline.best_gt_iou(qd, torch.from_numpy(offsets), gd, torch.from_numpy(frame), max_workgroups=3)
    want, want_idx = _best_by_numpy(qd, offsets, gd, frame)
    empty = counts[frame] == 0
    assert empty.sum() >= 3 and np.isnan(v3.cpu().numpy()[empty]).all() and np.all(idx.cpu().numpy()[empty] == -1)
    assert np.isnan(vb.cpu().numpy()[empty]).all()
    assert np.array_equal(bits(v3)[~empty], want.view(np.uint32)[~empty])
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(bits(v3b), bits(v3)) and np.array_equal(idxb.cpu().numpy(), idx.cpu().numpy())
    assert (want[~empty] > 0.3).mean() > 0.8
