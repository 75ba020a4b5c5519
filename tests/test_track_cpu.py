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
