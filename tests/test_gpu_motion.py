"""The motion-state kernels on the device (dal3_group_by_key / dal3_track_features / dal3_gt_table /
dal3_motion_classify) against NumPy (tests/motion_ref.py) and against what the reference's trackGT.py / motionState.py
recorded (tests/golden/motion.npz); the resident path from a TrackResult to SegmentPlan tracks."""
import importlib

import numpy as np
import pytest
import torch

import motion_ref
from _common import golden

motion = importlib.import_module("3dal_pytorch_amd.motion")
trk = importlib.import_module("3dal_pytorch_amd.track")
hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-9                                                 # tests/test_motion_cpu.py derives it


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name, spec in (("train", motion_ref.TRAIN), ("val", motion_ref.VAL)):
        frames, tracks = motion_ref.scene(**spec)
        gt = motion_ref.gt_table(frames)
        flat = motion.flatten_tracks(tracks, gt)
        # the entries in frame order (as trackData.pkl lists them), not track after track
        frame_of = {fr["token"]: i for i, fr in enumerate(frames)}
        fi = np.array([frame_of[t] for o in tracks.values() for t in o["token"]])
        perm = np.argsort(fi, kind="stable")
        out[name] = (frames, tracks, gt, {k: np.ascontiguousarray(v[perm]) for k, v in flat.items()})
    return out


def _same(a, b):
    return a.shape == b.shape and bool((a == b).all())


def test_group_by_key_is_the_stable_argsort_on_the_fixture(scenes):
    for name in ("train", "val"):
        _, tracks, _, flat = scenes[name]
        g = motion.group_by_key(dev(flat["keys"]), len(tracks))
        g.check()
        assert np.array_equal(g.entry.cpu().numpy(), np.argsort(flat["keys"], kind="stable"))
        assert np.array_equal(np.diff(g.group_start.cpu().numpy()), np.bincount(flat["keys"], minlength=len(tracks)))
        assert int(g.n_groups.item()) == len(tracks)


def test_group_by_key_large_any_grid_any_run():
    keys, T, empty, single, long = motion_ref.big_keys(11)
    assert len(keys) >= 5_000_000
    d = dev(keys)
    a = motion.group_by_key(d, T)
    b = motion.group_by_key(d, T, max_workgroups=7)
    c = motion.group_by_key(d, T)
    a.check()
    for other in (b, c):                                    # two grid sizes, two runs: the same bits
        assert torch.equal(a.entry, other.entry) and torch.equal(a.group_start, other.group_start)
    start, entry = a.group_start.cpu().numpy(), a.entry.cpu().numpy()
    assert np.array_equal(entry, np.argsort(keys, kind="stable").astype(np.int32))
    n = np.diff(start)
    assert np.array_equal(n, np.bincount(keys, minlength=T))
    assert (n[empty] == 0).all() and n[single] == 1 and n[long] == 198


@pytest.mark.parametrize("T", (1, 255, 256, 65536))
@pytest.mark.parametrize("E", (1, 255, 256, 257, 4095, 4096, 4097, 8193))
def test_group_by_key_at_the_tile_chunk_and_pass_edges(E, T):
    """keys in [0, T] take 1 (T = 1, 255), 2 (256) and 3 (65536) radix passes; E crosses the 256-entry tile and the
    4096-entry chunk, so the last tile is full, ragged or a single entry. At most five distinct keys: the order inside
    a key is decided by position alone."""
    rng = np.random.default_rng(E * 100_003 + T)
    keys = rng.integers(0, T, 5)[rng.integers(0, 5, E)].astype(np.int64)
    want = np.argsort(keys, kind="stable").astype(np.int32)
    d = dev(keys)
    for wg in (0, 1):
        g = motion.group_by_key(d, T, max_workgroups=wg)
        g.check()
        assert np.array_equal(g.entry.cpu().numpy(), want), wg
        assert np.array_equal(np.diff(g.group_start.cpu().numpy()), np.bincount(keys, minlength=T)), wg
        assert int(g.n_groups.item()) == int(keys.max()) + 1


@pytest.mark.parametrize("E", (257, 4097))
def test_group_by_key_at_four_passes(E):
    """T = 2^24 (DAL3_MAX_ITEMS) is the one T whose keys take four radix passes: the positions swap buffers an even number
    of times and must still end in `entry`. The keys differ in every digit; E is just past the tile and just past the
    chunk. Kept apart from the edges above: group_start is 128 MiB at this T."""
    T = 1 << 24
    rng = np.random.default_rng(E)
    keys = np.array([0, 255, 256, 65536, T - 1], np.int64)[rng.integers(0, 5, E)]
    want = np.argsort(keys, kind="stable").astype(np.int32)
    sizes = np.bincount(keys, minlength=T)
    d = dev(keys)
    for wg in (0, 1):
        g = motion.group_by_key(d, T, max_workgroups=wg)
        g.check()
        assert np.array_equal(g.entry.cpu().numpy(), want), wg
        assert np.array_equal(np.diff(g.group_start.cpu().numpy()), sizes), wg
        assert int(g.n_groups.item()) == int(keys.max()) + 1


@pytest.mark.parametrize("T", (1023, 1024, 1025, 2049))
def test_classify_ids_at_the_compaction_tile_edges(T):
    """a compaction tile is 1024 groups, ranked 256 at a time: one tile short of full, full, one group into the second,
    one into the third; about half the groups kept"""
    rng = np.random.default_rng(T)
    feat, keep = rng.normal(0, 1, (T, 2)), (rng.uniform(0, 1, T) < 0.5).astype(np.uint8)
    model = (np.array([0.7, -1.3]), 0.05)
    d = feat[:, 0] * model[0][0] + feat[:, 1] * model[0][1] + model[1]
    for wg in (0, 1):
        c = motion.classify(dev(feat), dev(keep), model, max_workgroups=wg)
        s, dyn = c.ids()
        assert np.array_equal(s, np.flatnonzero((keep > 0) & (d > 0))), wg
        assert np.array_equal(dyn, np.flatnonzero((keep > 0) & ~(d > 0))), wg
        assert c.counts.cpu().tolist() == [len(s), len(dyn)]


def test_group_by_key_bad_key_empty_input_and_no_groups():
    keys = np.array([3, 1, 99, 1, -5, 0, 3], np.int64)
    g = motion.group_by_key(dev(keys), 4)
    with pytest.raises(RuntimeError, match="DAL3_MOTION_BAD_KEY"):
        g.check()
    want_start, want_entry = motion_ref.group(keys, 4)
    n = int(want_start[-1])
    assert np.array_equal(g.group_start.cpu().numpy(), want_start)
    assert np.array_equal(g.entry.cpu().numpy()[:n], want_entry)
    e = motion.group_by_key(torch.zeros(0, dtype=torch.int64, device=DEV), 5)
    e.check()
    assert e.group_start.cpu().tolist() == [0] * 6 and int(e.n_groups.item()) == 0
    z = motion.group_by_key(torch.zeros(0, dtype=torch.int64, device=DEV), 0)
    z.check()
    assert z.group_start.cpu().tolist() == [0]
    f = motion.track_features(e, torch.zeros((0, 3), dtype=torch.float64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                              torch.zeros(0, dtype=torch.float32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                              torch.zeros(0, dtype=torch.int32, device=DEV))
    assert f.n.cpu().tolist() == [0] * 5 and f.keep.cpu().tolist() == [0] * 5
    c = motion.classify(f.feature, f.keep, (np.array([1.0, 1.0]), 0.5))
    assert c.counts.cpu().tolist() == [0, 0]
    c0 = motion.classify(torch.zeros((0, 2), dtype=torch.float64, device=DEV), torch.zeros(0, dtype=torch.uint8, device=DEV),
                         (np.array([1.0, 1.0]), 0.5))
    assert c0.counts.cpu().tolist() == [0, 0]


def test_group_by_key_key_base_and_frame_slots():
    """ids counted from a device base, frames with unused tail slots (a TrackResult's layout)"""
    rng = np.random.default_rng(5)
    counts, used = rng.integers(0, 40, 300), []
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    keys = rng.integers(-2**40, 2**40, int(off[-1])).astype(np.int64)           # the tails hold anything
    want = np.full(len(keys), -1, np.int64)
    for f in range(300):
        u = int(rng.integers(0, counts[f] + 1))
        used.append(u)
        ids = 1000 + 1 + rng.integers(0, 500, u)
        keys[off[f]:off[f] + u] = ids
        want[off[f]:off[f] + u] = ids - 1001
    g = motion.group_by_key(dev(keys), 500, key_base=dev(np.array([1000], np.int64)), key_bias=1, frame_offsets=dev(off),
                            out_count=dev(np.array(used, np.int32)))
    g.check()
    start, entry = motion_ref.group(want, 500)
    assert np.array_equal(g.group_start.cpu().numpy(), start)
    assert np.array_equal(g.entry.cpu().numpy()[:start[-1]], entry)


def test_track_features_against_numpy_and_the_recorded_features(scenes):
    g = golden("motion")
    for name in ("train", "val"):
        _, tracks, gt, flat = scenes[name]
        T = len(tracks)
        groups = motion.group_by_key(dev(flat["keys"]), T)
        f = motion.track_features(groups, dev(flat["center"]), dev(flat["type"]), dev(flat["score"]), dev(flat["n_points"]),
                                  dev(flat["match"]))
        groups.check()
        start, entry = motion_ref.group(flat["keys"], T)
        want = motion_ref.features(start, entry, flat["center"], flat["type"], flat["score"], flat["n_points"], flat["match"])
        for k in ("n", "type0", "match_last", "points_sum", "best", "keep"):      # integers, keep, argmax: exact
            assert np.array_equal(getattr(f, k).cpu().numpy(), want[k]), k
        keep = want["keep"].astype(bool)
        assert [k for k, kept in zip(tracks, keep) if kept] == list(g[f"{name}_keep_ids"])
        got, ref = f.feature.cpu().numpy()[keep], g[f"{name}X"]
        rel = np.abs(got - ref) / np.abs(ref)
        print(f"{name}: max relative error of the float64 features vs the reference {rel.max():.3e} "
              f"(distance {rel[:, 0].max():.3e}, variance {rel[:, 1].max():.3e}; eps = 2.2e-16)")
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0)
        np.testing.assert_allclose(f.feature.cpu().numpy(), want["feature"], rtol=RTOL, atol=0)
        static = np.array([o["static"] for o in gt.values()])
        assert np.array_equal(static[f.match_last.cpu().numpy()[keep]], g[f"{name}Y"])


def _gt_inputs(frames):
    key_of, keys, rows, frame = {}, [], [], []
    for f, fr in enumerate(frames):
        for obj in fr["objects"]:
            keys.append(key_of.setdefault(obj["name"], len(key_of)))
            rows.append(np.asarray(obj["box"], np.float64))
            frame.append(f)
    return len(key_of), np.array(keys, np.int64), np.array(rows), np.array(frame, np.int32), np.array([fr["pose"] for fr in frames])


def test_gt_table_static_flags_are_the_reference_ones(scenes):
    g = golden("motion")
    for name in ("train", "val"):
        T, keys, rows, frame, pose = _gt_inputs(scenes[name][0])
        groups = motion.group_by_key(dev(keys), T)
        t = motion.gt_table(groups, dev(rows), dev(frame), dev(pose))
        groups.check()
        assert np.array_equal(t.is_static.cpu().numpy(), g[f"gt_{name}_static"])          # exact
        assert np.array_equal(t.n.cpu().numpy(), g[f"gt_{name}_len"])
        # dist is a difference of 1e4 m coordinates: absolute 1e-11 m; the speeds were recorded in float32
        np.testing.assert_allclose(t.dist.cpu().numpy(), g[f"gt_{name}_dist"], rtol=RTOL, atol=1e-10)
        np.testing.assert_allclose(t.max_vel.cpu().numpy(), g[f"gt_{name}_max_vel"], rtol=1e-6, atol=1e-7)
        first = groups.entry.cpu().numpy()[groups.group_start.cpu().numpy()[:-1]]
        np.testing.assert_allclose(t.box_global.cpu().numpy()[first], g[f"gt_{name}_first_box"], rtol=RTOL, atol=1e-12)
    bad = motion.gt_table(groups, dev(rows), dev(np.full(len(rows), len(pose), np.int32)), dev(pose))
    with pytest.raises(RuntimeError, match="DAL3_MOTION_BAD_KEY"):
        groups.check()
    assert bool(torch.isnan(bad.vel).all())


def _val_features(scenes):
    _, tracks, _, flat = scenes["val"]
    groups = motion.group_by_key(dev(flat["keys"]), len(tracks))
    return tracks, motion.track_features(groups, dev(flat["center"]), dev(flat["type"]), dev(flat["score"]), dev(flat["n_points"]),
                                         dev(flat["match"]))


def test_classify_with_the_recorded_model_reproduces_the_prediction(scenes):
    g = golden("motion")
    tracks, f = _val_features(scenes)
    c = motion.classify(f.feature, f.keep, (g["coef"], float(g["intercept"][0])))
    keep = f.keep.cpu().numpy().astype(bool)
    d, ref = c.decision.cpu().numpy()[keep], g["decision"]
    assert np.abs(d - ref).max() <= 1e-3 * (1 + np.abs(ref)).min()                       # the same model: far inside
    clear = np.abs(ref) > 2e-3
    assert (~clear).mean() <= 0.01
    assert np.array_equal(c.is_static.cpu().numpy()[keep][clear], g["y_pred"][clear])
    ids = list(tracks.keys())
    s, dyn = c.ids()
    if clear.all():                                                                      # the order of the reference's dicts
        assert [ids[i] for i in s] == list(g["val_trackStatic_ids"])
        assert [ids[i] for i in dyn] == list(g["val_trackDynamic_ids"])
    # the compaction is stable and complete whatever the labels are
    lab = c.is_static.cpu().numpy().astype(bool)
    assert np.array_equal(s, np.nonzero(keep & lab)[0]) and np.array_equal(dyn, np.nonzero(keep & ~lab)[0])
    c2 = motion.classify(f.feature, f.keep, (g["coef"], float(g["intercept"][0])), max_workgroups=1)
    assert torch.equal(c.static_ids[:len(s)], c2.static_ids[:len(s)]) and torch.equal(c.decision, c2.decision)


def test_fit_on_the_train_features_then_classify_on_the_device(scenes):
    """libsvm's own stop (tol = 1e-3) is the yardstick: |d_ours - d_ref| <= 1e-3 (1 + |d_ref|) on every val row, equal
    labels on every val row with |d_ref| > 2e-3"""
    g = golden("motion")
    _, f = _val_features(scenes)
    w, b = motion.fit_linear_svm(g["trainX"], g["trainY"])
    c = motion.classify(f.feature, f.keep, (w, b))
    keep = f.keep.cpu().numpy().astype(bool)
    d, ref = c.decision.cpu().numpy()[keep], g["decision"]
    err = np.abs(d - ref) / (1 + np.abs(ref))
    print(f"svm on the device: max |d - d_ref| / (1 + |d_ref|) = {err.max():.3e}")
    assert err.max() <= 1e-3
    clear = np.abs(ref) > 2e-3
    assert (~clear).mean() <= 0.01
    assert np.array_equal(c.is_static.cpu().numpy()[keep][clear], g["y_pred"][clear])


def test_compaction_over_many_tiles():
    rng = np.random.default_rng(9)
    T = 300_001
    feat, keep = rng.normal(0, 1, (T, 2)), (rng.uniform(0, 1, T) < 0.6).astype(np.uint8)
    model = (np.array([0.7, -1.3]), 0.05)
    a = motion.classify(dev(feat), dev(keep), model)
    b = motion.classify(dev(feat), dev(keep), model, max_workgroups=3)
    d = feat[:, 0] * model[0][0] + feat[:, 1] * model[0][1] + model[1]
    assert np.array_equal(a.decision.cpu().numpy(), d)
    s, dyn = a.ids()
    assert np.array_equal(s, np.nonzero((keep > 0) & (d > 0))[0]) and np.array_equal(dyn, np.nonzero((keep > 0) & ~(d > 0))[0])
    s2, dyn2 = b.ids()
    assert np.array_equal(s, s2) and np.array_equal(dyn, dyn2)


def _shuffled_sequence():
    """tests/test_gpu_track_files.py's shuffled-detections input: 6 objects over 7 frames, each frame shuffled"""
    rng = np.random.default_rng(71)
    F, n = 7, 6
    p0, v = rng.uniform(-20, 20, (n, 2)), rng.uniform(-3, 3, (n, 2))
    frames = []
    for f in range(F):
        perm = rng.permutation(n)
        pos = p0 + v * 0.1 * f
        box = np.concatenate([pos, np.full((n, 1), 0.5), np.full((n, 3), 2.0), v, np.zeros((n, 1))], axis=1)[perm]
        frames.append({"frame_id": f, "timestamp": 0.1 * f, "box3d": box.astype(np.float32), "label": np.zeros(n, np.int64),
                       "score": rng.uniform(0.8, 1.0, n).astype(np.float32), "pose": np.eye(4).reshape(16)})
    return frames, n, float(np.median(np.linalg.norm(v, axis=1)) * 0.1 * (F - 1))


def _entry_arrays(res, frames, n_points=5, match=None):
    det = motion.detection_index(res)
    centre = np.concatenate([fr["box3d"][:, :3] for fr in frames]).astype(np.float64)
    score = np.concatenate([fr["score"] for fr in frames])
    E = len(score)
    return (dev(centre)[det], torch.ones(E, dtype=torch.int32, device=DEV), dev(score)[det],
            torch.full((E,), n_points, dtype=torch.int32, device=DEV),
            torch.zeros(E, dtype=torch.int32, device=DEV) if match is None else match)


def test_tracks_equal_segment_tracks_on_shuffled_detections():
    frames, n, median_path = _shuffled_sequence()
    inp = trk.TrackInputs(frames)
    res = trk.track_sequences(**inp.to(DEV))
    model = (np.array([-1.0, 0.0]), median_path)            # the slower half static, the faster half dynamic
    out = motion.motion_state(res, *_entry_arrays(res, frames), model)
    kinds = out.kinds()
    assert len(kinds) == n and set(kinds.values()) == {"static", "dynamic"}
    want = trk.segment_tracks(res.frames(), kinds, [fr["score"] for fr in frames])
    got = out.tracks([fr["score"] for fr in frames])
    assert got == want
    assert [t["id"] for t in got] == sorted(kinds)
    # a frame range: the same as segment_tracks on those frames alone
    sub = out.tracks([fr["score"] for fr in frames[2:6]], frame_range=(2, 6))
    assert sub == trk.segment_tracks(res.frames()[2:6], kinds, [fr["score"] for fr in frames[2:6]])
    # the best-score position is np.argmax over the track's scores
    best = out.features.best.cpu().numpy()
    for t in got:
        assert best[t["id"] - 1] == int(np.argmax(np.stack(t["score"])))


def test_no_host_sync_from_the_tracker_result_to_the_classes():
    frames, n, _ = _shuffled_sequence()
    inp = trk.TrackInputs(frames)
    res = trk.track_sequences(**inp.to(DEV), capacity=inp.capacity(3))
    arrays = _entry_arrays(res, frames)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        groups = motion.group_tracks(res, capacity=64)
        feats = motion.track_features(groups, *arrays)
        cls = motion.classify(feats.feature, feats.keep, (np.array([-2.0, -0.5]), 1.0))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    motion.MotionResult(groups, feats, cls, res).check()
    assert int(cls.counts.sum().item()) == n and int(groups.n_groups.item()) == n


def test_a_segment_plan_built_from_the_motion_result_runs():
    """tracker -> motion state -> SegmentPlan on the segment of tests/test_gpu_pipeline.py with every frame's detections
    shuffled: every object becomes one track of 7 detections and every tracked detection is rewritten"""
    from _common import build_model, synth
    from test_gpu_pipeline import _segment
    segment = importlib.import_module("3dal_pytorch_amd.segment")
    crops = importlib.import_module("3dal_pytorch_amd.crops")
    poses, sweeps, dets, gbox = _segment(n_frames=7, n_obj=6, seed=71)
    rng = np.random.default_rng(2)
    dets = [d[rng.permutation(len(d))] for d in dets]
    F, K = len(poses), gbox.shape[0]
    frames = [{"frame_id": f, "timestamp": 0.1 * f, "box3d": dets[f], "label": np.zeros(K, np.int64),
               "score": rng.uniform(0.8, 1.0, K).astype(np.float32), "pose": poses[f]} for f in range(F)]
    inp = trk.TrackInputs(frames)
    res = trk.track_sequences(**inp.to(DEV))
    det = motion.detection_index(res)
    centre = np.concatenate([crops.transform_box(crops.waymo_boxes(d), np.reshape(p, [4, 4]))[:, :3] for d, p in zip(dets, poses)])
    E = len(centre)
    ones = torch.ones(E, dtype=torch.int32, device=DEV)
    out = motion.motion_state(res, dev(centre.astype(np.float64))[det], ones, dev(np.concatenate([fr["score"] for fr in frames]))[det],
                              ones, ones, (np.array([-2.0, -0.5]), 1.0))
    tracks = out.tracks([fr["score"] for fr in frames])
    assert len(tracks) == K and all(t["kind"] == "static" and len(t["dets"]) == F for t in tracks)    # parked objects
    tracks[1]["kind"] = tracks[3]["kind"] = "dynamic"                                  # both heads
    plan = segment.SegmentPlan([s.shape[0] for s in sweeps], dets, poses, tracks, build_model("static_one", synth.state_dict("static_one")),
                               build_model("dynamic", synth.state_dict("dynamic")), n_static_points=1024, n_per_frame=256)
    r = plan.run(torch.from_numpy(np.concatenate(sweeps)).cuda())
    torch.cuda.synchronize()
    assert not plan.overflowed()
    assert bool((r["static"][1] >= 0).all()) and bool((r["dynamic"][1] >= 0).all())
    assert r["static"][1].numel() == 4 * F and r["dynamic"][1].numel() == 2 * F
