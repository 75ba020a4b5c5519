"""dal3_track / dal3_track_match where they can go wrong: the seeded inputs of tests/track_ref.py that contend, tie,
carry NaN and inf, sit on the score and age thresholds, on the wave (64), block (256) and bitmap-word (32) edges and past
the match kernels' grid cap of 65,535 frames — against the NumPy restatement (track_ref.track / track_ref.match with
tests/iou_ref.py), which tests/test_track_cpu.py holds to the reference's own tracker on the same inputs. Every
comparison is of integers and exact."""
import functools
import importlib

import numpy as np
import pytest
import torch

import iou_ref
import track_ref

trk = importlib.import_module("3dal_pytorch_amd.track")
hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
AGES = (0, 1, 2, 3)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev(ct, tr, lab, sc, fo, so):
    return dict(seq_offsets=_t(so), frame_offsets=_t(fo), ct=_t(ct), tracking=_t(tr), label=_t(lab.astype(np.int32)),
                score=_t(sc.astype(np.float32)))


def _same(got, want):
    assert len(got) == len(want)
    for f, ((b, t), (wb, wt)) in enumerate(zip(got, want)):
        assert np.array_equal(b, wb) and np.array_equal(t, wt), f


def _seqs(inputs, s0, s1):
    """sequences [s0, s1) of an input, as an input of its own"""
    ct, tr, lab, sc, fo, so = inputs
    f0, f1 = int(so[s0]), int(so[s1])
    k0, k1 = int(fo[f0]), int(fo[f1])
    return ct[k0:k1], tr[k0:k1], lab[k0:k1], sc[k0:k1], fo[f0:f1 + 1] - k0, so[s0:s1 + 1] - f0


def _concat(a, b):
    return tuple(np.concatenate([x, y]) for x, y in zip(a[:4], b[:4])) + (
        np.concatenate([a[4], b[4][1:] + a[4][-1]]), np.concatenate([a[5], b[5][1:] + a[5][-1]]))


def _raw_frames(res):
    """TrackResult.frames() without its check(): for runs whose status is set on purpose"""
    off, cnt = res.frame_offsets.cpu().numpy(), res.out_count.cpu().numpy()
    b, t = res.box_ids.cpu().numpy().astype(np.int64), res.tracking_ids.cpu().numpy()
    return [(b[off[f]:off[f] + cnt[f]], t[off[f]:off[f] + cnt[f]]) for f in range(len(cnt))]


# ------------------------------------------------------------------------------------ the scenes and their parameters
def _scenes():
    """{name: (inputs, parameters but max_age)}: every input of track_ref's second half once"""
    out = {}
    for name, (inputs, params) in track_ref.dense_cases().items():
        if name.startswith("threshold_age"):
            name = "threshold"
        out.setdefault(name, (inputs, {k: v for k, v in params.items() if k != "max_age"}))
    out["many_frames"] = (track_ref.many_frames(), {})
    return out


SCENES = _scenes()


@functools.lru_cache(maxsize=None)
def _want(name, max_age):
    inputs, params = SCENES[name]
    with np.errstate(invalid="ignore"):
        return track_ref.track(*inputs, max_age=max_age, **params)


@functools.lru_cache(maxsize=None)
def _max_live(name, max_age=3):
    inputs, params = SCENES[name]
    return track_ref.stats(*inputs, max_age=max_age, **params)["max_live"]


@pytest.mark.parametrize("max_age", AGES)
@pytest.mark.parametrize("name", list(SCENES))
def test_tracker_kernel_equals_the_restatement(name, max_age):
    inputs, params = SCENES[name]
    want, ids = _want(name, max_age)
    res = trk.track_sequences(**_dev(*inputs), max_age=max_age, **params)
    _same(res.frames(), want)
    assert res.total() == ids


# ---------------------------------------------------------------------------------- the launch and the batch split
def _split_cases():
    ring = track_ref.tie_ring()
    return {"crowded": (SCENES["crowded"][0], 1), "crowded_far": (SCENES["crowded_far"][0], 2), "tie_ring": (_concat(ring, ring), 1)}


@pytest.mark.parametrize("name", ["crowded", "crowded_far", "tie_ring"])
def test_result_does_not_depend_on_the_grid_or_the_batch_split(name):
    inputs, cut = _split_cases()[name]
    want, ids = track_ref.track(*inputs)
    full = trk.track_sequences(**_dev(*inputs))
    _same(full.frames(), want)
    for wg in (1, 2):
        res = trk.track_sequences(**_dev(*inputs), max_workgroups=wg)
        _same(res.frames(), want)
        assert res.total() == ids
    S = len(inputs[5]) - 1
    a = trk.track_sequences(**_dev(*_seqs(inputs, 0, cut)))
    b = trk.track_sequences(**_dev(*_seqs(inputs, cut, S)), id_base=a.id_total)
    _same(a.frames() + b.frames(), want)
    assert b.total() == ids


def test_no_sequence_returns_the_id_base():
    base = torch.tensor([4711], dtype=torch.int64, device=DEV)
    res = trk.track_sequences(**_dev(*SCENES["edge_S0"][0]), id_base=base)
    assert res.frames() == [] and res.total() == 4711
    assert trk.track_sequences(**_dev(*SCENES["edge_S0"][0])).total() == 0


# -------------------------------------------------------------------------------------------------------- capacity
@pytest.mark.parametrize("name", ["crowded", "crowded_far", "continuous", "continuous_far"])
def test_capacity_at_the_largest_live_list_and_one_below(name):
    inputs, _ = SCENES[name]
    live = _max_live(name)
    res = trk.track_sequences(**_dev(*inputs), capacity=live)
    assert int(res.status.item()) == 0
    _same(res.frames(), _want(name, 3)[0])
    assert res.total() == _want(name, 3)[1]
    res = trk.track_sequences(**_dev(*inputs), capacity=live - 1)
    assert int(res.status.item()) == hip.TRACK_OVERFLOW
    with pytest.raises(RuntimeError, match="capacity"):
        res.frames()


def test_an_overflowing_sequence_leaves_the_others_alone():
    inputs = track_ref.crowded_scene(23, seqs=((330, 8), (150, 6)))
    alone = _seqs(inputs, 1, 2)
    cap = track_ref.stats(*alone)["max_live"]                   # enough for the second sequence only
    assert cap < track_ref.stats(*_seqs(inputs, 0, 1))["max_live"]
    res = trk.track_sequences(**_dev(*inputs), capacity=cap)
    assert int(res.status.item()) == hip.TRACK_OVERFLOW
    got = _raw_frames(res)[int(inputs[5][1]):]
    want, n_ids = track_ref.track(*alone)
    assert len(got) == len(want)
    shift = {int(x) for (b, t), (wb, wt) in zip(got, want) for x in t - wt}     # ids up to the common offset
    assert len(shift) == 1
    for (b, t), (wb, wt) in zip(got, want):
        assert np.array_equal(b, wb)


# ------------------------------------------------------------------------------------------------------ a bad label
@pytest.mark.parametrize("bad", [3, -1])
def test_a_label_outside_the_classes_sets_the_status(bad):
    inputs = track_ref.crowded_scene(24, seqs=((60, 4), (90, 5)))
    ct, tr, lab, sc, fo, so = inputs
    lab = lab.copy()
    first = int(fo[so[1]])                                      # the second sequence starts here
    lab[[0, 7, first - 1]] = bad                                # the first sequence: its first frame and its last row
    res = trk.track_sequences(**_dev(ct, tr, lab, sc, fo, so))
    assert int(res.status.item()) == hip.TRACK_BAD_LABEL
    with pytest.raises(RuntimeError, match="label"):
        res.check()
    got = _raw_frames(res)[int(so[1]):]
    want, _ = track_ref.track(*_seqs(inputs, 1, 2))
    assert len({int(x) for (b, t), (wb, wt) in zip(got, want) for x in t - wt}) == 1
    for (b, t), (wb, wt) in zip(got, want):
        assert np.array_equal(b, wb)


# -------------------------------------------------------------------------------------------------- the match kernel
MATCH_SEED = 48
MATCH_THR = (0.75, 0.5)
G0_FRAMES, NAN_GT_FRAME, DUP_FRAME, LATE_UNTIL = (11, 25), 16, 20, 3


@functools.lru_cache(maxsize=None)
def _match_scene():
    """track_ref.scene at a few thousand detections (its NaN translation is the NaN detection box), with planted:
    frames without annotations, a NaN annotation box (no row of that frame matches), an annotation box repeated bitwise
    behind itself (the first index wins), and one track, seen in every frame of the second sequence, whose annotation
    boxes are removed from its first LATE_UNTIL frames (None until its first candidate, that (frame, object) after)."""
    frames = track_ref.scene(MATCH_SEED, n_obj=150, clutter=40)
    inp = trk.TrackInputs(frames)
    inputs = (inp.ct, inp.tracking, inp.label, inp.score, inp.frame_offsets, inp.seq_offsets)
    with np.errstate(invalid="ignore"):
        tracked, ids = track_ref.track(*inputs)
    fo = inp.frame_offsets
    boxes = np.concatenate([trk.crops.waymo_boxes(fr["box3d"]) for fr in frames]).astype(np.float32)
    gts = [fr["gt"][:, [0, 1, 2, 3, 4, 5, -1]].astype(np.float32) for fr in frames]
    iou = lambda f: iou_ref.pairwise(boxes[fo[f]:fo[f + 1]].astype(np.float64), gts[f].astype(np.float64))[1]   # noqa: E731
    for f in G0_FRAMES:
        gts[f] = gts[f][:0]
    gts[NAN_GT_FRAME][3, 1] = np.nan
    v = np.nan_to_num(iou(DUP_FRAME))
    dup = int(np.argmax(v.max(axis=0)))                         # an annotation box that some detection matches
    assert v[:, dup].max() > 0.8
    gts[DUP_FRAME] = np.concatenate([gts[DUP_FRAME], gts[DUP_FRAME][dup:dup + 1]])
    # the late track: the first id seen in every frame of the second sequence (the first one's NaN track stops every
    # match for max_age frames) with a candidate LATE_UNTIL frames or more after its birth at the stricter threshold
    n0, n1 = int(inp.seq_offsets[1]), int(inp.seq_offsets[2])
    pre = {f: np.nan_to_num(iou(f)) for f in range(n0, n1)}
    late = None
    for tid in tracked[n0][1]:
        rows = {f: tracked[f][0][tracked[f][1] == tid] for f in range(n0, n1)}
        if all(len(r) == 1 for r in rows.values()) and any(pre[f][rows[f][0]].max() > 0.8 for f in range(n0 + LATE_UNTIL, n1)
                                                           if f != NAN_GT_FRAME and f not in G0_FRAMES):
            late = int(tid)
            for f in range(n0, n0 + LATE_UNTIL):
                gts[f] = gts[f][~(pre[f][rows[f][0]] > 0)]
            break
    assert late is not None
    goff = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int64)
    return inputs, tracked, ids, boxes, np.concatenate(gts), goff, late


def _expected_match(tracked, boxes, fo, gt, goff, thr):
    m = track_ref.match(tracked, boxes, fo, gt, goff, lambda a, b: iou_ref.pairwise(a, b)[1], thr=thr)
    flat = [x for row in m for x in row]
    return np.array([-1 if x is None else x[0] for x in flat]), np.array([-1 if x is None else x[1] for x in flat]), m


def _positions(fo, tracked):
    return np.concatenate([np.arange(fo[f], fo[f] + len(b)) for f, (b, _) in enumerate(tracked)] + [np.zeros(0, np.int64)]).astype(np.int64)


def test_match_scene_keeps_its_margins_and_holds_the_planted_cases():
    """conditions on the input, from the float64 IoUs (no GPU work): a float32 IoU then decides as float64 does"""
    inputs, tracked, ids, boxes, gt, goff, late = _match_scene()
    fo = inputs[4]
    assert 3000 < len(boxes) < 9000
    for f, (b, _) in enumerate(tracked):
        g = gt[goff[f]:goff[f + 1]]
        if len(g) == 0 or not np.isfinite(g).all():
            continue
        v = iou_ref.pairwise(boxes[fo[f]:fo[f + 1]][b].astype(np.float64), g.astype(np.float64))[1]
        for r in range(len(b)):
            if not np.isfinite(v[r]).all():
                continue
            order = np.argsort(-v[r], kind="stable")
            best = v[r, order[0]]
            for thr in MATCH_THR:
                assert abs(best - thr) > 1e-5, (f, r, best)
            # two best within 1e-5 only where the boxes are the same bits. A row whose best IoU is itself within 1e-5
            # of 0 cannot meet that (the zeros of every far box are as close) and has no candidate at any threshold
            if len(order) > 1 and best > 1e-5 and best - v[r, order[1]] <= 1e-5:
                assert np.array_equal(g[order[0]], g[order[1]]), (f, r, best, v[r, order[1]])
    assert all(goff[f + 1] == goff[f] for f in G0_FRAMES)
    assert np.isnan(gt[goff[NAN_GT_FRAME]:goff[NAN_GT_FRAME + 1]]).sum() == 1
    nan_det = np.nonzero(~np.isfinite(boxes).all(1))[0]
    assert len(nan_det) == 1
    f_nan = int(np.searchsorted(fo, nan_det[0], side="right") - 1)
    assert nan_det[0] - fo[f_nan] in tracked[f_nan][0]                      # the NaN box is a tracked detection
    for thr in MATCH_THR:
        mf, mo, m = _expected_match(tracked, boxes, fo, gt, goff, thr)
        assert all(x is None or x[0] < NAN_GT_FRAME for x in m[NAN_GT_FRAME]) and len(m[NAN_GT_FRAME]) > 50   # no new match
        assert m[f_nan][tracked[f_nan][0].tolist().index(nan_det[0] - fo[f_nan])] is None
        g = gt[goff[DUP_FRAME]:goff[DUP_FRAME + 1]]
        first = [j for j in range(len(g) - 1) if np.array_equal(g[j], g[-1])][0]
        hits = [x for x in m[DUP_FRAME] if x is not None and x[0] == DUP_FRAME]
        assert (DUP_FRAME, first) in hits and (DUP_FRAME, len(g) - 1) not in hits      # the first of the equal boxes wins
        n0, n1 = int(inputs[5][1]), int(inputs[5][2])
        track_of = [m[f][tracked[f][1].tolist().index(late)] for f in range(n0, n1)]
        k = [x is not None for x in track_of].index(True)
        assert k >= LATE_UNTIL and all(x == track_of[k] for x in track_of[k:]) and track_of[k][0] == n0 + k
        assert (mo >= 0).sum() > 500


@pytest.mark.parametrize("thr", MATCH_THR)
def test_match_kernel_equals_the_restatement(thr):
    inputs, tracked, ids, boxes, gt, goff, _ = _match_scene()
    fo, so = inputs[4], inputs[5]
    want_f, want_o, _ = _expected_match(tracked, boxes, fo, gt, goff, thr)
    res = trk.track_sequences(**_dev(*inputs))
    mf, mo = trk.match_ground_truth(res, _t(boxes), _t(goff), _t(gt), thr=thr)
    _same(res.frames(), tracked)                                            # the match is of the GPU tracker's own output
    pos = _positions(fo, tracked)
    assert np.array_equal(mf.cpu().numpy()[pos], want_f) and np.array_equal(mo.cpu().numpy()[pos], want_o)
    # two batches, the ids continuing, each matched on its own: frames and object indices are the batch's
    cut = 1
    f_cut = int(so[cut])
    k_cut, g_cut = int(fo[f_cut]), int(goff[f_cut])
    a = trk.track_sequences(**_dev(*_seqs(inputs, 0, cut)))
    b = trk.track_sequences(**_dev(*_seqs(inputs, cut, len(so) - 1)), id_base=a.id_total)
    amf, amo = trk.match_ground_truth(a, _t(boxes[:k_cut]), _t(goff[:f_cut + 1]), _t(gt[:g_cut]), thr=thr)
    bmf, bmo = trk.match_ground_truth(b, _t(boxes[k_cut:]), _t(goff[f_cut:] - g_cut), _t(gt[g_cut:]), thr=thr)
    a.check()
    b.check()
    n_a = int((pos < k_cut).sum())
    assert np.array_equal(amf.cpu().numpy()[pos[:n_a]], want_f[:n_a]) and np.array_equal(amo.cpu().numpy()[pos[:n_a]], want_o[:n_a])
    wf_b = np.where(want_f[n_a:] >= 0, want_f[n_a:] - f_cut, -1)
    assert np.array_equal(bmf.cpu().numpy()[pos[n_a:] - k_cut], wf_b) and np.array_equal(bmo.cpu().numpy()[pos[n_a:] - k_cut], want_o[n_a:])


def test_match_kernel_reports_ids_outside_the_range():
    inputs, tracked, ids, boxes, gt, goff, _ = _match_scene()
    res = trk.track_sequences(**_dev(*inputs))
    res.check()
    for base in (10 ** 6, -10 ** 6):
        moved = trk.TrackResult(res.frame_offsets, res.box_ids, res.tracking_ids, res.out_count, res.id_total,
                                torch.zeros(1, dtype=torch.int32, device=DEV), torch.tensor([base], dtype=torch.int64, device=DEV))
        mf, mo = trk.match_ground_truth(moved, _t(boxes), _t(goff), _t(gt))
        assert int(moved.status.item()) == hip.TRACK_BAD_ID
        with pytest.raises(RuntimeError, match="BAD_ID"):
            moved.check()
        assert (mo.cpu().numpy() == -1).all()


def test_match_kernel_past_the_grid_cap():
    """many_frames: one annotation box per frame — a copy of one of the frame's detection boxes or a box far away — so
    the expectation needs no IoU: an entry is a candidate iff it is the copied detection, and an id matches from its
    first candidate on"""
    inputs = SCENES["many_frames"][0]
    ct, fo = inputs[0], inputs[4]
    tracked, ids = _want("many_frames", 3)
    F, K = len(fo) - 1, len(ct)
    assert F > 65535
    rng = np.random.default_rng(5)
    boxes = np.concatenate([ct, np.zeros((K, 1)), np.tile([4.0, 2.0, 1.5], (K, 1)), rng.uniform(-3, 3, (K, 1))], axis=1).astype(np.float32)
    pick = fo[:-1] + rng.integers(0, 2, F) % np.diff(fo)                     # the detection each frame's box copies
    far = rng.uniform(0, 1, F) < 0.3
    gt = boxes[pick].copy()
    gt[far, :2] += 1000.0
    goff = np.arange(F + 1, dtype=np.int64)
    cnt = np.array([len(b) for b, _ in tracked])
    frame = np.repeat(np.arange(F), cnt)
    pos = _positions(fo, tracked)
    det = fo[frame] + np.concatenate([b for b, _ in tracked])                # the detection of every output entry
    tid = np.concatenate([t for _, t in tracked])
    cand = (det == pick[frame]) & ~far[frame]
    first = np.full(ids + 1, np.iinfo(np.int64).max)
    np.minimum.at(first, tid[cand], np.nonzero(cand)[0])                     # entries are in position order
    hit = first[tid] <= np.arange(len(tid))
    want_f = np.where(hit, frame[np.minimum(first[tid], len(tid) - 1)], -1)
    assert hit.sum() > 20000 and (~hit).sum() > 20000 and (hit & ~cand).sum() > 1000
    res = trk.track_sequences(**_dev(*inputs))
    mf, mo = trk.match_ground_truth(res, _t(boxes), _t(goff), _t(gt))
    _same(res.frames(), tracked)
    assert np.array_equal(mf.cpu().numpy()[pos], want_f)
    assert np.array_equal(mo.cpu().numpy()[pos], np.where(hit, 0, -1))
