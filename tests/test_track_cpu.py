"""The tracking run without a GPU: the NumPy restatement (tests/track_ref.py) against the reference's own PubTracker
and the restated `matching` loop (tests/golden/tracking.npz, exact), the CLI's host logic (the global-frame inputs,
the frame order, the train ratio and split, the id strings, trackData.py's regroup) and the C header's new entries."""
import importlib
import os
import re

import numpy as np

import iou_ref
import track_ref
from _common import ROOT, golden

trk = importlib.import_module("3dal_pytorch_amd.track")
hip = importlib.import_module("3dal_pytorch_amd._hip")
SEED = 2024


def _scene():
    return track_ref.scene(SEED)


def _per_frame(g):
    off = np.concatenate([[0], np.cumsum(g["out_count"])])
    return [(g["box_ids"][off[f]:off[f + 1]], g["tracking_ids"][off[f]:off[f + 1]]) for f in range(len(off) - 1)]


def test_global_inputs_are_the_reference_bits():
    g = golden("tracking")
    inp = trk.TrackInputs(_scene())
    assert np.array_equal(inp.ct, g["ct"], equal_nan=True)
    vel = np.concatenate([trk.global_ct_velocity(fr["box3d"], fr["pose"])[1] for fr in _scene()])
    assert np.array_equal(vel, g["velocity"])


def test_restated_tracker_equals_the_reference_pubtracker():
    g = golden("tracking")
    inp = trk.TrackInputs(_scene())
    out, ids = track_ref.track(inp.ct, inp.tracking, inp.label, inp.score, inp.frame_offsets, inp.seq_offsets)
    want = _per_frame(g)
    assert len(out) == len(want)
    for (b, t), (wb, wt) in zip(out, want):
        assert np.array_equal(b, wb) and np.array_equal(t, wt)
    assert ids == int(g["id_count"])
    # the cases the fixture is meant to pin are present
    assert (g["out_count"] == 0).any()
    assert len(inp.seq_offsets) - 1 == 3
    assert np.isnan(inp.ct).any()


def test_restated_match_equals_the_fixture():
    g = golden("tracking")
    frames = _scene()
    inp = trk.TrackInputs(frames)
    boxes = np.concatenate([trk.crops.waymo_boxes(fr["box3d"]) for fr in frames]).astype(np.float32)
    gts = [fr["gt"][:, [0, 1, 2, 3, 4, 5, -1]] for fr in frames]
    goff = np.concatenate([[0], np.cumsum([len(x) for x in gts])])
    m = track_ref.match(_per_frame(g), boxes, inp.frame_offsets, np.concatenate(gts), goff,
                        lambda a, b: iou_ref.pairwise(a, b)[1])
    flat = [x for row in m for x in row]
    assert np.array_equal([-1 if x is None else x[0] for x in flat], g["match_frame"])
    assert np.array_equal([-1 if x is None else x[1] for x in flat], g["match_obj"])
    assert (g["match_obj"] >= 0).sum() > 50


def test_frame_order_ratio_split_and_ids():
    toks = [fr["token"] for fr in _scene()]
    shuffled = [toks[i] for i in np.random.default_rng(1).permutation(len(toks))]
    assert [shuffled[r] for r in trk.sort_order(shuffled)] == toks
    assert trk.frame_key("seq_12_frame_7.pkl") == 12007
    d = {f"k{i}": i for i in range(37)}
    parts = trk.split_dict(dict(list(d.items())[:int(37 * 0.25)]), 16)
    assert len(parts) == 16 and sum(len(p) for p in parts) == 9
    assert [k for p in parts for k in p] == [f"k{i}" for i in range(9)]
    ids = {trk.object_id(t) for t in range(1, 500)}
    assert len(ids) == 499 and all(re.fullmatch(r"[0-9a-f]{32}", i) for i in ids)


def test_regroup_equals_trackdata_py():
    g = golden("tracking")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_tracking", os.path.join(ROOT, "tests", "golden", "gen_tracking.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    td = gen.regroup_input(_per_frame(g), [fr["token"] for fr in _scene()])
    tr = trk.regroup(td)
    assert list(tr.keys()) == list(g["regroup_ids"])
    assert ["|".join(v["token"]) for v in tr.values()] == list(g["regroup_tokens"])
    assert np.array_equal(np.concatenate([np.asarray(v["score"], np.float64) for v in tr.values()]), g["regroup_scores"])


def test_capacity_bound_covers_the_restated_run():
    ct, tr, lab, sc, fo, so = track_ref.big_scene(5, n_seq=12)
    counts = np.diff(fo)
    inp = trk.TrackInputs.__new__(trk.TrackInputs)
    inp.counts, inp.seq_offsets = counts, so
    assert inp.capacity(3) >= 700


def test_header_declares_the_tracking_entries():
    text = open(os.path.join(ROOT, "include", "dal3.h")).read()
    assert int(re.search(r"^#define\s+DAL3_VERSION\s+(\d+)", text, re.M).group(1)) == hip.lib().dal3_version()
    for name in ("dal3_track_workspace_bytes", "dal3_track", "dal3_track_match_workspace_bytes", "dal3_track_match"):
        assert re.search(rf"\b{name}\(", text), name
        assert name in hip.SIGNATURES
    for name in ("dal3_track_args", "dal3_track_match_args", "DAL3_TRACK_MAX_CAPACITY", "DAL3_TRACK_OVERFLOW"):
        assert name in text
    assert int(re.search(r"#define DAL3_TRACK_MAX_CAPACITY (\d+)", text).group(1)) == hip.TRACK_MAX_CAPACITY


# ------------------------------------------------------------------ the dense scenes (tests/golden/tracking_dense.npz)
# Recorded from the reference's PubTracker: every case of track_ref.dense_cases(), the 27 (N, M) pairs included.
# track_ref.many_frames() is NOT recorded (100 k entries of a two-detection pattern): it is held to the restatement alone.
_CASES = track_ref.dense_cases()
_STATS = {}


def _stats(name):
    if name not in _STATS:
        inputs, params = _CASES[name] if name in _CASES else (track_ref.many_frames(), {})
        _STATS[name] = track_ref.stats(*inputs, **params)
    return _STATS[name]


def _track(name):
    inputs, params = _CASES[name]
    with np.errstate(invalid="ignore"):
        return track_ref.track(*inputs, **params)


def test_restated_tracker_equals_the_reference_on_every_dense_scene():
    g = golden("tracking_dense")
    assert sorted({k.split("__")[0] for k in g}) == sorted(_CASES)
    for name in _CASES:
        out, ids = _track(name)
        assert np.array_equal([len(b) for b, _ in out], g[name + "__out_count"]), name
        assert np.array_equal(np.concatenate([b for b, _ in out] + [np.zeros(0, np.int64)]), g[name + "__box_ids"]), name
        assert np.array_equal(np.concatenate([t for _, t in out] + [np.zeros(0, np.int64)]), g[name + "__tracking_ids"]), name
        assert ids == int(g[name + "__id_count"]), name


def test_crowded_scenes_contend_and_tie():
    """conditions on the inputs, from the restatement alone: about half of what the scenes give"""
    for name in ("crowded", "crowded_far", "continuous", "continuous_far"):
        s = _stats(name)
        assert s["rescanned"] >= 0.25 * s["rows"], (name, s["rescanned"], s["rows"])
        assert s["matches"] >= 0.5 * s["rows"], (name, s["matches"], s["rows"])
        assert s["max_n"] > 256 and s["max_live"] > 256, name
    for name in ("crowded", "crowded_far"):
        assert _stats(name)["ties"] >= 0.1 * _stats(name)["rows"], name
    keys = ("rows", "rescanned", "ties", "max_n", "max_m", "matches", "max_live")
    assert [_stats("crowded")[k] for k in keys] == [_stats("crowded_far")[k] for k in keys]   # exact at 3e5 m alike
    assert _stats("continuous")["ties"] == 0
    assert _stats("continuous_far")["ties"] >= 1
    # three sequences of different size in one call; the second's list passes 64 and stays below 256
    ct, tr, lab, sc, fo, so = _CASES["crowded"][0]
    assert len(so) == 4
    mid = tuple(a[fo[so[1]]:fo[so[2]]] for a in (ct, tr, lab, sc)) + (fo[so[1]:so[2] + 1] - fo[so[1]], np.array([0, so[2] - so[1]]))
    assert 64 < track_ref.stats(*mid)["max_live"] < 256
    # detections are multiples of 1/8 m: exact in float32 at the origin and at 3e5 m
    far = _CASES["crowded_far"][0][0]
    assert np.array_equal(ct * 8, np.round(ct * 8)) and np.array_equal(far.astype(np.float32).astype(np.float64), far)
    assert np.array_equal(far - 300000.0, ct)


def test_tie_ring_ties_at_the_designed_columns():
    s = _stats("tie_ring_default")
    for pair in track_ref.TIE_RING_PAIRS:
        assert tuple(pair) in s["tie_sets"], pair
    assert tuple(track_ref.TIE_RING_MANY) in s["tie_sets"]
    for k in range(1, len(track_ref.TIE_RING_MANY) - 1):                # every later row: the free columns that remain
        assert tuple(track_ref.TIE_RING_MANY[k:]) in s["tie_sets"], k
    assert s["max_m"] >= track_ref.TIE_RING_M and s["rescanned"] >= 15
    (b1, t1) = _track("tie_ring_default")[0][1]
    took = dict(zip(b1.tolist(), (t1 - 1).tolist()))                    # frame 1: row -> column (id - 1) where matched
    M = track_ref.TIE_RING_M
    assert [took[r] for r in (0, 1, 2)] == [5, 6, 69] and took[3] >= M              # rows at a, b, a; a third at a: none left
    assert [took[r] for r in (4, 5)] == [63, 64] and took[6] >= M
    assert [took[r] for r in (7, 10)] == [0, M - 1] and took[11] >= M
    assert [took[r] for r in (8, 9)] == [31, 32]
    assert [took[r] for r in range(12, 24)] == list(track_ref.TIE_RING_MANY) and took[24] >= M and took[25] >= M
    # max_dist exactly the ring distance still matches; the float32 just below it matches nothing on a ring
    exact, below = _track("tie_ring_exact"), _track("tie_ring_below")
    assert np.array_equal(exact[0][1][1], t1) and exact[1] == _track("tie_ring_default")[1]
    assert (below[0][1][1] > M).all() and _stats("tie_ring_below")["ties"] == 0
    assert track_ref.TIE_RING_MAX_DIST["below"][0] < 0.625 == track_ref.TIE_RING_MAX_DIST["exact"][0]


def test_nonfinite_scene_decides_as_its_comment_says():
    out, ids = _track("nonfinite")
    rows = lambda f: out[f][0].tolist()         # noqa: E731
    tids = lambda f: out[f][1].tolist()         # noqa: E731
    assert (rows(1), tids(1)) == ([0, 1, 2, 3, 6, 4, 5], [1, 2, 3, 4, 6, 9, 10])     # the NaN rows: no match, new tracks
    for f in (2, 3, 4):                                                             # two NaN tracks live: nothing matches
        assert rows(f) == [0, 1, 2] and tids(f) == list(range(11 + 3 * (f - 2), 14 + 3 * (f - 2)))
    assert (rows(5), tids(5)) == ([0, 1, 2, 3, 4, 5], [17, 18, 19, 20, 21, 22])      # gone after max_age frames
    assert tids(6) == tids(5)
    assert tids(7) == [23, 24, 25, 26, 27, 28]                                      # 28: the inf track
    assert (rows(8), tids(8)) == ([0, 3, 4, 5, 6, 1, 2], [23, 24, 25, 26, 27, 29, 30])   # NaN score (row 7): no id
    assert tids(9) == [23, 24, 25, 26, 27] and ids == 30
    ct, _, _, sc, fo, so = _CASES["nonfinite"][0]
    assert np.isnan(ct).sum() == 2 and np.isinf(ct).sum() == 3 and np.isnan(sc).sum() == 1
    assert _stats("nonfinite")["rescanned"] >= 2                                    # the NaN rows' column 0 was taken


def test_threshold_scene_decides_as_its_comment_says():
    s75, s_next, s6 = track_ref.THRESHOLD_SCORES
    assert float(s75) == 0.75 and float(s_next) > 0.75 and float(s6) > 0.6 and s6 == np.float32(0.6)
    first = lambda name, row: [t for b, t in zip(*_track(name)[0][0]) if b == row]   # noqa: E731
    assert first("threshold_age3", 0) == [] and first("threshold_age3", 1) == [1] and first("threshold_age3", 2) == []
    assert first("threshold_0.6", 0) == [1] and first("threshold_0.6", 2) == [3]
    for max_age in (0, 1, 2, 3):
        out, _ = _track(f"threshold_age{max_age}")
        born = dict(zip(out[0][0].tolist(), out[0][1].tolist()))        # frame 0: row -> id; object h is row 3 + h
        for h in track_ref.THRESHOLD_HIDDEN[1:]:
            b, t = out[h + 1]                                           # the frame object h returns in, as row 3 + (h - 1)... by id
            kept = born[3 + h] in t.tolist()
            assert kept == (h < max_age), (max_age, h)
        for f in range(len(out)):                                       # the two objects always seen keep their ids
            assert born[8] in out[f][1] and born[9] in out[f][1]


def test_edge_layouts_are_what_they_claim():
    e = track_ref.edge_layouts()
    assert len(e["S0"][5]) == 1 and len(e["S0"][4]) == 1
    assert len(e["K0"][2]) == 0 and len(e["K0"][4]) == 4
    assert e["no_frames"][5].tolist() == [0, 0, 2, 2, 4, 4]
    counts = lambda k: np.diff(e[k][4]).tolist()        # noqa: E731
    assert counts("first_empty")[2] == 0 and e["first_empty"][5].tolist() == [0, 2, 5, 6]
    assert counts("all_empty")[2:4] == [0, 0] and e["all_empty"][5].tolist() == [0, 2, 4, 6]
    assert counts("single") == [1]
    c = np.array(counts("pairs")).reshape(-1, 2)
    assert [(int(n), int(m)) for m, n in c] == list(track_ref.EDGE_NM) and len(track_ref.EDGE_NM) == 27
    out, _ = _track("edge_pairs")
    assert all(len(out[2 * q][0]) == m for q, (n, m) in enumerate(track_ref.EDGE_NM))   # frame 0 leaves M tracks
    assert _stats("edge_pairs")["rescanned"] > 1000


def test_many_frames_passes_the_grid_cap():
    ct, tr, lab, sc, fo, so = track_ref.many_frames()
    assert len(fo) - 1 == 66000 > 65535 and len(so) - 1 == 33000 > 256
    assert set(np.diff(fo).tolist()) == {1, 2}
    s = _stats("many_frames")
    assert s["matches"] > 10000 and s["rows"] - s["matches"] > 5000


def test_capacity_bound_covers_every_dense_scene():
    for name in list(_CASES) + ["many_frames"]:
        inputs, params = _CASES[name] if name in _CASES else (track_ref.many_frames(), {})
        max_age = params.get("max_age", 3)
        inp = trk.TrackInputs.__new__(trk.TrackInputs)
        inp.counts, inp.seq_offsets = np.diff(inputs[4]), inputs[5]
        assert inp.capacity(max_age) >= _stats(name)["max_live"], name
    for max_age in (0, 1, 2):                   # the crowded scene at every max_age
        inputs = _CASES["crowded"][0]
        inp = trk.TrackInputs.__new__(trk.TrackInputs)
        inp.counts, inp.seq_offsets = np.diff(inputs[4]), inputs[5]
        assert inp.capacity(max_age) >= track_ref.stats(*inputs, max_age=max_age)["max_live"], max_age
