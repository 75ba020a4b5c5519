"""The tracking run on the device: CenterPoint's greedy tracker (tools/waymo_tracking/test.py + tracker.py, PubTracker)
over every frame of every sequence in one launch (dal3_track), the ground-truth match of
`_create_pd_detection(tracking=True)` (det3d/datasets/waymo/waymo_common.py:67-218; dal3_track_match), the crops of
the tracked detections (crops.extract_crops) and the regrouping of tools/trackData.py.

    python -m 3dal_pytorch_amd.track --work_dir W --checkpoint P --info_path I [--max_age 3 --vehicle 0.8
        --pedestrian 0.4 --cyclist 0.6 --score_thresh 0.75]
    python -m 3dal_pytorch_amd.track regroup --work_dir W [--split 16]

writes what test.py / trackData.py write: det_annos.pkl, trackData.pkl (a `val` work dir) or trackData_{i}.pkl x 16
(a `train` work dir, the first 25 % of the frames), and for `regroup` track.pkl / track_{i}.pkl.

Host work is what the reference does per frame in NumPy (the detections moved to the global frame, test.py:150-249,
vectorised per frame with the reference's own expressions, so the float64 inputs are its bits) and the pickles.

Deliberate departures:
- no tracking_pred.bin: the Waymo protos are not available;
- object ids are deterministic 32-hex strings of the tracking id (`object_id`), not uuid4 (random in the reference,
  so there are no values to match; downstream code only compares ids for equality);
- a frame whose tracker output is empty writes empty arrays (the reference's `[np.array([])]` index fails there).
"""
import argparse
import os
import pickle
import sys

import numpy as np
import torch

from . import _hip, crops
from .eval import Annos, reorganize_info

NAMES = ["VEHICLE", "PEDESTRIAN", "CYCLIST"]
LABEL_TO_TYPE = {0: 1, 1: 2, 2: 4}                          # waymo_common.py:40
LABEL_TO_NAME = {0: "Vehicle", 1: "Pedestrian", 2: "Cyclist"}


def object_id(tracking_id):
    """the trackData 'id' of a tracking id: 32 hex digits (the reference's uuid4().hex has the same form)"""
    return f"{int(tracking_id):032x}"


def frame_key(token):
    """sort key of test.py:sort_detections (:190-205): seq_id * 1000 + frame_id of 'seq_{s}_frame_{f}.pkl'"""
    parts = token.split("_")
    return int(parts[1]) * 1000 + int(parts[3][:-4])


def sort_order(tokens):
    """the frame order of sort_detections (the same np.argsort call)"""
    return [int(r) for r in np.argsort(np.array([frame_key(t) for t in tokens]))]


def transform_box9(box, pose):
    """test.py:150-170 (the 9-column transform that also rotates the velocity) for (K,9) boxes and one 4x4 pose"""
    heading = box[..., -1] + np.arctan2(pose[..., 1, 0], pose[..., 0, 0])
    center = np.einsum("...ij,...nj->...ni", pose[..., 0:3, 0:3], box[..., 0:3]) + np.expand_dims(pose[..., 0:3, 3], axis=-2)
    velocity = box[..., [6, 7]]
    velocity = np.concatenate([velocity, np.zeros((velocity.shape[0], 1))], axis=-1)
    velocity = np.einsum("...ij,...nj->...ni", pose[..., 0:3, 0:3], velocity)[..., [0, 1]]
    return np.concatenate([center, box[..., 3:6], velocity, heading[..., np.newaxis]], axis=-1)


def global_ct_velocity(box3d_lidar, pose):
    """convert_detection_to_global_box (test.py:219-221) for one frame: (K,9) float32 detector boxes -> ct (K,2),
    velocity (K,2), float64"""
    box3d = np.array(box3d_lidar, dtype=np.float32, copy=True).reshape(-1, 9)
    box3d[:, -1] = -box3d[:, -1] - np.pi / 2
    box3d[:, [3, 4]] = box3d[:, [4, 3]]
    g = transform_box9(box3d, np.reshape(np.asarray(pose, np.float64), [4, 4]))
    return np.ascontiguousarray(g[:, :2]), np.ascontiguousarray(g[:, [6, 7]])


class TrackInputs:
    """The flat tracker inputs of frames already in tracking order. frames: list of dicts with 'frame_id',
    'timestamp', 'box3d' (K,9) float32, 'label' (K) int, 'score' (K) float32, 'pose' (flat-16 veh_to_global).
    test.py:84-101: frame_id == 0 starts a sequence (tracks reset, time_lag 0); tracking = velocity * -1 * time_lag."""

    def __init__(self, frames):
        if frames and frames[0]["frame_id"] != 0:
            raise ValueError("track: the first frame must have frame_id 0 (the reference's loop has no time_lag before it)")
        ct, tr, lab, sc, counts, starts = [], [], [], [], [], []
        last = None
        for f, fr in enumerate(frames):
            if fr["frame_id"] == 0:
                starts.append(f)
                last = fr["timestamp"]
            time_lag = fr["timestamp"] - last
            last = fr["timestamp"]
            c, v = global_ct_velocity(fr["box3d"], fr["pose"])
            labels = np.asarray(fr["label"]).astype(np.int32).reshape(-1)
            if labels.size and (labels.min() < 0 or labels.max() > 2):
                raise ValueError("track: labels must be 0..2 (VEHICLE, PEDESTRIAN, CYCLIST)")
            ct.append(c)
            tr.append(v * -1 * time_lag)
            lab.append(labels)
            sc.append(np.asarray(fr["score"], np.float32).reshape(-1))
            counts.append(c.shape[0])
        cat = lambda xs, shape, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt)   # noqa: E731
        self.ct = cat(ct, (0, 2), np.float64)
        self.tracking = cat(tr, (0, 2), np.float64)
        self.label = cat(lab, (0,), np.int32)
        self.score = cat(sc, (0,), np.float32)
        self.counts = np.asarray(counts, np.int64)
        self.frame_offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.seq_offsets = np.asarray(starts + [len(frames)], np.int64)

    def capacity(self, max_age):
        """live tracks any frame can hold: the most detections in max(max_age, 1) consecutive frames of a sequence"""
        w = max(int(max_age), 1)
        best = 1
        for s in range(len(self.seq_offsets) - 1):
            c = self.counts[self.seq_offsets[s]:self.seq_offsets[s + 1]]
            if c.size:
                cs = np.concatenate([[0], np.cumsum(c)])
                best = max(best, int((cs[w:] - cs[:-w]).max()) if c.size >= w else int(cs[-1]))
        return best

    def to(self, device):
        dev = torch.device(device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        return {"seq_offsets": t(self.seq_offsets), "frame_offsets": t(self.frame_offsets), "ct": t(self.ct),
                "tracking": t(self.tracking), "label": t(self.label), "score": t(self.score)}


class TrackResult:
    """dal3_track's outputs, device tensors: frame f's entries are box_ids / tracking_ids[frame_offsets[f] :
    frame_offsets[f] + out_count[f]]; id_total = the tracker's id_count after the run; status the device word."""

    def __init__(self, frame_offsets, box_ids, tracking_ids, out_count, id_total, status, id_base):
        self.frame_offsets, self.box_ids, self.tracking_ids = frame_offsets, box_ids, tracking_ids
        self.out_count, self.id_total, self.status, self.id_base = out_count, id_total, status, id_base

    def check(self):
        """raise if the device reported a problem (a host sync)"""
        st = int(self.status.item())
        if st & _hip.TRACK_OVERFLOW:
            raise RuntimeError("track: a sequence holds more live tracks than the capacity (dal3_track status "
                               "DAL3_TRACK_OVERFLOW); its ids are not a result — run again with a larger capacity")
        if st & _hip.TRACK_BAD_LABEL:
            raise RuntimeError("track: a detection label outside 0..2 (dal3_track status DAL3_TRACK_BAD_LABEL)")
        if st & _hip.TRACK_BAD_ID:
            raise RuntimeError("track: a tracking id outside the run's range (status DAL3_TRACK_BAD_ID)")

    def total(self):
        return int(self.id_total.item())

    def frames(self):
        """per frame (box_ids int64, tracking_ids int64) NumPy arrays — test.py's box_ids / tracking_ids lists"""
        self.check()
        off = self.frame_offsets.cpu().numpy()
        cnt = self.out_count.cpu().numpy()
        b, t = self.box_ids.cpu().numpy().astype(np.int64), self.tracking_ids.cpu().numpy()
        return [(b[off[f]:off[f] + cnt[f]], t[off[f]:off[f] + cnt[f]]) for f in range(len(cnt))]


def track_sequences(seq_offsets, frame_offsets, ct, tracking, label, score, max_age=3, max_dist=(0.8, 0.4, 0.6),
                    score_thresh=0.75, capacity=None, id_base=None, max_workgroups=0):
    """PubTracker.step_centertrack over every frame of every sequence, one dal3_track call on the current stream.
    Device tensors in (TrackInputs.to): seq_offsets (S+1) / frame_offsets (F+1) int64, ct / tracking (K,2) float64,
    label (K) int32, score (K) float32. max_dist per class (VEHICLE, PEDESTRIAN, CYCLIST). capacity: live tracks per
    sequence (TrackInputs.capacity gives the bound that always suffices; without one, the offsets are read back ONCE to
    form it — the only host sync, absent when a capacity is given). id_base: optional device int64 (1) — ids continue
    after it, e.g. a previous result's id_total. Returns a TrackResult whose check() / frames() read the status."""
    dev = ct.device
    S, F, K = seq_offsets.numel() - 1, frame_offsets.numel() - 1, ct.shape[0]
    if not capacity:
        b = TrackInputs.__new__(TrackInputs)
        b.counts, b.seq_offsets = np.diff(frame_offsets.cpu().numpy()), seq_offsets.cpu().numpy()
        capacity = min(b.capacity(max_age), _hip.TRACK_MAX_CAPACITY)
    cap = int(capacity)
    lib = _hip.lib()
    ws = _hip.workspace(lib.dal3_track_workspace_bytes(S, K, cap), dev)
    box_ids = torch.empty(max(K, 1), dtype=torch.int32, device=dev)
    tracking_ids = torch.empty(max(K, 1), dtype=torch.int64, device=dev)
    out_count = torch.empty(max(F, 1), dtype=torch.int32, device=dev)
    id_total = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    a = _hip.TrackArgs()
    a.S, a.F, a.K = S, F, K
    a.seq_offsets, a.frame_offsets = _hip.ptr(seq_offsets), _hip.ptr(frame_offsets)
    a.ct, a.tracking, a.label, a.score = _hip.ptr(ct), _hip.ptr(tracking), _hip.ptr(label), _hip.ptr(score)
    for c in range(3):
        a.max_dist[c] = float(max_dist[c])
    a.max_age, a.score_thresh, a.capacity, a.max_workgroups = int(max_age), float(score_thresh), cap, int(max_workgroups)
    a.id_base = _hip.ptr(id_base)
    a.box_ids, a.tracking_ids, a.out_count = _hip.ptr(box_ids), _hip.ptr(tracking_ids), _hip.ptr(out_count)
    a.id_total, a.status = _hip.ptr(id_total), _hip.ptr(status)
    a.workspace, a.workspace_bytes = _hip.ptr(ws), ws.numel()
    _hip.check(lib.dal3_track(a, _hip.stream()))
    return TrackResult(frame_offsets, box_ids, tracking_ids, out_count[:F], id_total, status, id_base)


def match_ground_truth(result, boxes, gt_offsets, gt_boxes, thr=0.75):
    """The `match` of _create_pd_detection (waymo_common.py:173-189) for every output entry of `result`: boxes (K,7)
    float32 device, Waymo convention (crops.waymo_boxes), by detection in frame order; gt_offsets (F+1) int64,
    gt_boxes (G,7) float32 device (obj['box'][[0,1,2,3,4,5,-1]] of each frame). Returns (match_frame, match_obj) int32
    device tensors by output position (-1: None); result.status collects a bad id. No host sync."""
    dev = boxes.device
    F, K = result.out_count.numel(), boxes.shape[0]
    lib = _hip.lib()
    ws = _hip.workspace(lib.dal3_track_match_workspace_bytes(K), dev)
    mf = torch.full((max(K, 1),), -1, dtype=torch.int32, device=dev)
    mo = torch.full((max(K, 1),), -1, dtype=torch.int32, device=dev)
    gt = gt_boxes if gt_boxes.numel() else torch.zeros((1, 7), dtype=torch.float32, device=dev)
    a = _hip.TrackMatchArgs()
    a.F, a.K = F, K
    a.frame_offsets, a.out_count = _hip.ptr(result.frame_offsets), _hip.ptr(result.out_count)
    a.box_ids, a.tracking_ids, a.id_base = _hip.ptr(result.box_ids), _hip.ptr(result.tracking_ids), _hip.ptr(result.id_base)
    a.boxes, a.gt_offsets, a.gt_boxes, a.thr = _hip.ptr(boxes), _hip.ptr(gt_offsets), _hip.ptr(gt), float(thr)
    a.match_frame, a.match_obj, a.status = _hip.ptr(mf), _hip.ptr(mo), _hip.ptr(result.status)
    a.workspace, a.workspace_bytes = _hip.ptr(ws), ws.numel()
    _hip.check(lib.dal3_track_match(a, _hip.stream()))
    return mf, mo


def det_anno(labels, scores, boxes_lidar, anno, info):
    """one entry of det_annos.pkl (waymo_common.py:116-129), shared by this run and the detection run (dist_test.py): the
    names of the labels, the scores, the boxes already in Waymo's convention, and the frame's identity from its annotation
    file `anno` and its info"""
    frame_id = anno["frame_id"]
    return {"name": np.array([LABEL_TO_NAME[int(i)] for i in labels]), "score": scores, "boxes_lidar": boxes_lidar,
            "frame_id": "segment-" + anno["scene_name"] + f"_with_camera_labels_{frame_id:03d}",
            "metadata": {"context_name": anno["scene_name"], "timestamp_micros": int(str(info["timestamp"]).replace(".", ""))}}


def regroup(track_data):
    """tools/trackData.py:24-45: {token: per-frame lists} -> {object id: per-track lists + 'token'}"""
    tracking = {}
    for token, frame in track_data.items():
        for idx in range(len(frame["id"])):
            oid = frame["id"][idx]
            t = tracking.get(oid)
            if t is None:
                t = tracking[oid] = {"type": [], "bbox": [], "score": [], "point": [], "match": [], "token": []}
            for key in ("type", "bbox", "score", "point", "match"):
                t[key].append(frame[key][idx])
            t["token"].append(token)
    return tracking


def split_dict(d, split):
    """dict(items[len * i // split : len * (i + 1) // split]) for i in range(split) (waymo_common.py:204-208)"""
    items = list(d.items())
    return [dict(items[len(items) * i // split:len(items) * (i + 1) // split]) for i in range(split)]


def segment_tracks(frames, kinds, scores):
    """the tracker's output for ONE segment -> segment.SegmentPlan's `tracks`. frames: per frame (box_ids,
    tracking_ids) (TrackResult.frames() of the segment's frames); scores: per frame the detections' scores; kinds:
    {tracking id: "static" | "dynamic"} (motion-state classification is the caller's). Tracks in order of first
    appearance; ids missing from `kinds` are left out."""
    out = {}
    for f, (box_ids, tids) in enumerate(frames):
        for k, tid in zip(np.asarray(box_ids).tolist(), np.asarray(tids).tolist()):
            kind = kinds.get(tid)
            if kind is None:
                continue
            t = out.get(tid)
            if t is None:
                t = out[tid] = {"kind": kind, "dets": [], "score": [], "id": tid}
            t["dets"].append((f, k))
            t["score"].append(np.asarray(scores[f])[k])
    return list(out.values())


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def run(work_dir, checkpoint, info_path, max_age=3, vehicle=0.8, pedestrian=0.4, cyclist=0.6, score_thresh=0.75,
        device="cuda", ratio=0.25, split=16):
    """test.py:main + _create_pd_detection(tracking=True); returns {token: trackData frame} as written"""
    dev = torch.device(device)
    print("Deploy OK")
    predictions = _load(checkpoint)
    infos = reorganize_info(_load(info_path))
    annos = Annos(infos)
    tokens = list(infos.keys())
    order = sort_order(tokens)
    tokens = [tokens[r] for r in order]
    frames = []
    for tok in tokens:
        det, a = predictions[tok], annos(tok)
        frames.append({"frame_id": int(tok.split("_")[3][:-4]), "timestamp": infos[tok]["timestamp"],
                       "box3d": _np(det["box3d_lidar"]).astype(np.float32), "label": _np(det["label_preds"]),
                       "score": _np(det["scores"]).astype(np.float32), "pose": a["veh_to_global"]})
    print(f"Begin Tracking {len(frames)} frames\n")
    inp = TrackInputs(frames)
    res = track_sequences(**inp.to(dev), max_age=max_age, max_dist=(vehicle, pedestrian, cyclist),
                          score_thresh=score_thresh, capacity=min(inp.capacity(max_age), _hip.TRACK_MAX_CAPACITY))
    # _create_pd_detection: the GT match on the device, for the frames it keeps
    keep = len(tokens)
    if "train" in work_dir:
        keep = int(len(tokens) * ratio)
    boxes_w = np.concatenate([crops.waymo_boxes(fr["box3d"]) for fr in frames]).astype(np.float32) if frames else \
        np.zeros((0, 7), np.float32)
    gts = []
    for tok in tokens:
        objs = annos(tok)["objects"]
        b = np.array([o["box"] for o in objs], dtype=np.float32).reshape(-1, 9) if objs else np.zeros((0, 9), np.float32)
        gts.append(b[:, [0, 1, 2, 3, 4, 5, -1]])
    gt_off = np.concatenate([[0], np.cumsum([g.shape[0] for g in gts])]).astype(np.int64)
    mf, mo = match_ground_truth(res, torch.from_numpy(np.ascontiguousarray(boxes_w)).to(dev), torch.from_numpy(gt_off).to(dev),
                                torch.from_numpy(np.ascontiguousarray(np.concatenate(gts), np.float32)).to(dev))
    per_frame = res.frames()
    total = res.total()
    off, mf, mo = inp.frame_offsets, mf.cpu().numpy(), mo.cpu().numpy()
    os.makedirs(work_dir, exist_ok=True)
    print("Total track object:", total)
    # crops of the kept frames' tracked detections, one batch
    kept = range(keep)
    sweeps = [np.asarray(_load(infos[tokens[f]]["path"])["lidars"]["points_xyz"], np.float32).reshape(-1, 3) for f in kept]
    tracked = [frames[f]["box3d"][per_frame[f][0]].reshape(-1, 9) for f in kept]
    ext = crops.extract_crops(sweeps, tracked, [frames[f]["pose"] for f in kept], dev) if keep else []
    det_annos, track_data = [], {}
    for f in kept:
        tok, fr, a = tokens[f], frames[f], annos(tokens[f])
        box_ids, tids = per_frame[f]
        labels = np.asarray(fr["label"]).reshape(-1)[box_ids]
        scores = fr["score"][box_ids]
        box3d = ext[f]["boxes_lidar"]
        det_annos.append(det_anno(labels, scores, box3d, a, infos[tok]))
        n = len(box_ids)
        match = []
        for r in range(n):
            g_f, g_o = int(mf[off[f] + r]), int(mo[off[f] + r])
            match.append(None if g_f < 0 else annos(tokens[g_f])["objects"][g_o]["name"])
        track_data[tok] = {"id": [object_id(t) for t in tids], "type": [LABEL_TO_TYPE[int(l)] for l in labels],
                           "bbox": list(ext[f]["bbox"]), "score": list(scores), "point": ext[f]["point"].numpy_list(),
                           "match": match}
    with open(os.path.join(work_dir, "det_annos.pkl"), "wb") as fh:
        pickle.dump(det_annos, fh)
    print("Saved det_annos.pkl")
    if "train" in work_dir:
        for i, part in enumerate(split_dict(track_data, split)):
            with open(os.path.join(work_dir, f"trackData_{i}.pkl"), "wb") as fh:
                pickle.dump(part, fh)
    elif "val" in work_dir:
        with open(os.path.join(work_dir, "trackData.pkl"), "wb") as fh:
            pickle.dump(track_data, fh)
    else:
        raise NotImplementedError("Not supported.")
    return track_data


def run_regroup(work_dir, split=16):
    """tools/trackData.py:main"""
    name = work_dir.rstrip("/").split("/")[-1]
    if name == "train":
        track = {}
        for i in range(split):
            track.update(_load(os.path.join(work_dir, f"trackData_{i}.pkl")))
    elif name == "val":
        track = _load(os.path.join(work_dir, "trackData.pkl"))
    else:
        raise NotImplementedError("Not supported.")
    tracking = regroup(track)
    if name == "train":
        for i, part in enumerate(split_dict(tracking, split)):
            with open(os.path.join(work_dir, f"track_{i}.pkl"), "wb") as fh:
                pickle.dump(part, fh)
    else:
        with open(os.path.join(work_dir, "track.pkl"), "wb") as fh:
            pickle.dump(tracking, fh)
    return tracking


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if argv and argv[0] == "regroup":
        p = argparse.ArgumentParser(prog="3dal_pytorch_amd.track regroup")
        p.add_argument("--work_dir", help="Path to working dir.")
        p.add_argument("--split", type=int, default=16, help="Number of train split.")
        args = p.parse_args(argv[1:])
        run_regroup(args.work_dir, args.split)
        return
    p = argparse.ArgumentParser(description="Tracking Evaluation")
    p.add_argument("--work_dir", help="the dir to save logs and tracking results")
    p.add_argument("--checkpoint", help="the path to prediction file")
    p.add_argument("--info_path", type=str)
    p.add_argument("--max_age", type=int, default=3)
    p.add_argument("--vehicle", type=float, default=0.8)
    p.add_argument("--pedestrian", type=float, default=0.4)
    p.add_argument("--cyclist", type=float, default=0.6)
    p.add_argument("--score_thresh", type=float, default=0.75)
    args = p.parse_args(argv)
    run(args.work_dir, args.checkpoint, args.info_path, args.max_age, args.vehicle, args.pedestrian, args.cyclist,
        args.score_thresh)


if __name__ == "__main__":
    main()
