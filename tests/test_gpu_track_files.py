"""The tracking CLI (python -m 3dal_pytorch_amd.track) on a written sequence against the reference's tracker and
match (tests/golden/tracking.npz): ids up to renaming, types, boxes, scores, matches; `regroup` -> track.pkl; and
SegmentPlan tracks built by track.segment_tracks from shuffled detections."""
import importlib
import os
import pickle

import numpy as np
import pytest
import torch

import track_ref
from _common import golden

trk = importlib.import_module("3dal_pytorch_amd.track")
SEED = 2024
pytestmark = pytest.mark.gpu


def _waymo_transform_box(box, pose):
    """waymo_common.py:52-65 on one (1,7) box, as _create_pd_detection calls it"""
    heading = box[..., -1] + np.arctan2(pose[..., 1, 0], pose[..., 0, 0])
    center = np.einsum("...ij,...nj->...ni", pose[..., 0:3, 0:3], box[..., 0:3]) + np.expand_dims(pose[..., 0:3, 3], axis=-2)
    return np.squeeze(np.concatenate([center, box[..., 3:6], heading[..., np.newaxis]], axis=-1))


def write_sequence(root, frames):
    os.makedirs(os.path.join(root, "annos"), exist_ok=True)
    os.makedirs(os.path.join(root, "lidar"), exist_ok=True)
    rng = np.random.default_rng(3)
    preds, infos = {}, []
    for fr in frames:
        tok = fr["token"]
        preds[tok] = {"box3d_lidar": torch.from_numpy(fr["box3d"]), "scores": torch.from_numpy(fr["score"]),
                      "label_preds": torch.from_numpy(fr["label"])}
        objs = [{"name": n, "box": b} for n, b in zip(fr["names"], fr["gt"])]
        apath, lpath = os.path.join(root, "annos", tok), os.path.join(root, "lidar", tok)
        with open(apath, "wb") as f:
            pickle.dump({"scene_name": "synth", "frame_name": f"synth_{fr['frame_id']}", "frame_id": fr["frame_id"],
                         "veh_to_global": fr["pose"], "objects": objs}, f)
        b = np.nan_to_num(fr["box3d"][:, :3])
        pts = (np.repeat(b, 20, axis=0) + rng.uniform(-1.5, 1.5, (20 * len(b), 3))).astype(np.float32)
        with open(lpath, "wb") as f:
            pickle.dump({"lidars": {"points_xyz": pts}}, f)
        infos.append({"token": tok, "anno_path": apath, "path": lpath, "timestamp": fr["timestamp"]})
    infos = [infos[i] for i in np.random.default_rng(SEED).permutation(len(infos))]
    paths = {"checkpoint": os.path.join(root, "preds.pkl"), "info_path": os.path.join(root, "infos.pkl")}
    for key, obj in (("checkpoint", preds), ("info_path", infos)):
        with open(paths[key], "wb") as f:
            pickle.dump(obj, f)
    return paths


def test_cli_writes_the_reference_trackdata_and_regroups(tmp_path, capsys):
    g = golden("tracking")
    frames = track_ref.scene(SEED)
    paths = write_sequence(str(tmp_path / "data"), frames)
    wd = str(tmp_path / "val")
    trk.main(["--work_dir", wd, "--checkpoint", paths["checkpoint"], "--info_path", paths["info_path"]])
    assert f"Total track object: {int(g['id_count'])}" in capsys.readouterr().out
    with open(os.path.join(wd, "trackData.pkl"), "rb") as f:
        td = pickle.load(f)
    assert list(td.keys()) == [fr["token"] for fr in frames]
    off = np.concatenate([[0], np.cumsum(g["out_count"])])
    rename = {}
    for f, fr in enumerate(frames):
        rec = td[fr["token"]]
        box_ids, tids = g["box_ids"][off[f]:off[f + 1]], g["tracking_ids"][off[f]:off[f + 1]]
        assert len(rec["id"]) == len(tids)
        for oid, tid in zip(rec["id"], tids):
            assert rename.setdefault(oid, int(tid)) == int(tid)
        assert rec["type"] == [{0: 1, 1: 2, 2: 4}[int(fr["label"][k])] for k in box_ids]
        assert [float(s) for s in rec["score"]] == [float(fr["score"][k]) for k in box_ids]
        pose = np.reshape(fr["pose"], [4, 4])
        w = trk.crops.waymo_boxes(fr["box3d"])
        for r, k in enumerate(box_ids):
            assert np.array_equal(rec["bbox"][r], _waymo_transform_box(w[k][np.newaxis, ...], pose), equal_nan=True)
        for r in range(len(tids)):
            mf, mo = g["match_frame"][off[f] + r], g["match_obj"][off[f] + r]
            assert rec["match"][r] == (None if mf < 0 else frames[mf]["names"][mo])
            assert rec["point"][r].dtype == np.float64 and rec["point"][r].shape[1] == 3
    assert len(set(rename.values())) == len(rename)
    trk.main(["regroup", "--work_dir", wd])
    with open(os.path.join(wd, "track.pkl"), "rb") as f:
        tr = pickle.load(f)
    assert list(tr.keys()) == list(trk.regroup(td).keys())
    assert sum(len(v["token"]) for v in tr.values()) == int(g["out_count"].sum())


def test_segment_tracks_from_shuffled_detections_equal_the_hand_association():
    """one sequence of 6 objects moving over 7 frames, each frame's detections shuffled: the kernel's tracks, turned
    into SegmentPlan tracks, hold the same (frame, detection) pairs as the hand-associated plan"""
    rng = np.random.default_rng(71)
    F, n = 7, 6
    p0, v = rng.uniform(-20, 20, (n, 2)), rng.uniform(-3, 3, (n, 2))
    frames, perms = [], []
    for f in range(F):
        perm = rng.permutation(n)
        pos = p0 + v * 0.1 * f
        box = np.concatenate([pos, np.full((n, 1), 0.5), np.full((n, 3), 2.0), v, np.zeros((n, 1))], axis=1)[perm]
        frames.append({"frame_id": f, "timestamp": 0.1 * f, "box3d": box.astype(np.float32), "label": np.zeros(n, np.int64),
                       "score": np.full(n, 0.9, np.float32), "pose": np.eye(4).reshape(16)})
        perms.append(perm)
    inp = trk.TrackInputs(frames)
    res = trk.track_sequences(**inp.to("cuda")).frames()
    kinds = {t: ("static" if t % 2 else "dynamic") for t in range(1, n + 1)}
    tracks = trk.segment_tracks(res, kinds, [fr["score"] for fr in frames])
    assert len(tracks) == n
    for t in tracks:
        objs = {int(perms[f][k]) for f, k in t["dets"]}
        assert len(objs) == 1 and [f for f, _ in t["dets"]] == list(range(F))
        assert t["kind"] == kinds[t["id"]]
