#!/usr/bin/env python3
"""Generate tracking.npz from the REAL reference (jacky121298/3DAL_PyTorch):

    tracker  tools/waymo_tracking/tracker.py's PubTracker (NumPy only), driven as test.py's main loop drives it, on
             the detections that test.py's own convert_detection_to_global_box / transform_box (:150-249) move to the
             global frame. test.py is imported with stub modules for pyquaternion, nuscenes and
             det3d.datasets.waymo.waymo_common (missing here or dragging in missing packages; the tracking path does
             not use them). Inputs: tests/track_ref.scene(SEED), written as the pickles test.py reads.
    match    the `matching` loop of _create_pd_detection (waymo_common.py:173-189) restated (tests/track_ref.match)
             with tests/iou_ref.py's IoU in place of pcdet's boxes_iou3d_gpu (not vendored). No best IoU may lie
             within 1e-5 of 0.75 (checked here), so a float32 IoU decides the same way.
    regroup  tools/trackData.py run on a temp `val` dir holding a trackData.pkl built from the tracker's output.

    dense    tracking_dense.npz: PubTracker.step_centertrack driven directly on tests/track_ref.dense_cases() — inputs
             already in tracker form. A detection is a dict with translation (x, y, 0), velocity = -tracking, fed with
             time_lag 1.0 (`velocity * -1 * time_lag` is then `tracking` bit for bit), detection_name by its label and
             its score as a Python float of the same value: the reference compares `score > score_thresh` in float64
             under the NumPy 1.x it was written for, while NumPy 2 would round the threshold to a float32 score's type.
             reset() at each sequence start; outputs filtered by `active != 0` as above.

Stored: the reference's outputs only (the inputs are rebuilt from the seed). Run where the reference exists
(DAL3_REFERENCE, default /root/reference); an argument names another output directory:
    python tests/golden/gen_tracking.py [OUT_DIR]
"""
import io
import os
import pickle
import sys
import tempfile
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import iou_ref  # noqa: E402
import track_ref  # noqa: E402

REF = os.environ.get("DAL3_REFERENCE", "/root/reference")
SEED = 2024
PARAMS = dict(max_age=3, vehicle=0.8, pedestrian=0.4, cyclist=0.6, score_thresh=0.75)


def import_test_py():
    for name in ["pyquaternion", "nuscenes", "nuscenes.utils", "nuscenes.utils.geometry_utils", "det3d", "det3d.datasets",
                 "det3d.datasets.waymo", "det3d.datasets.waymo.waymo_common"]:
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
    sys.modules["pyquaternion"].Quaternion = None
    sys.modules["nuscenes.utils.geometry_utils"].transform_matrix = None
    sys.modules["det3d.datasets.waymo.waymo_common"]._create_pd_detection = None
    sys.path.insert(0, REF)
    from tools.waymo_tracking import test as tp
    from tools.waymo_tracking.tracker import PubTracker
    return tp, PubTracker


def write_inputs(root, frames, seed):
    """the predictions / infos / annos pickles of test.py (infos deliberately not in frame order)"""
    os.makedirs(os.path.join(root, "annos"), exist_ok=True)
    preds, infos = {}, []
    for fr in frames:
        tok = fr["token"]
        preds[tok] = {"box3d_lidar": torch.from_numpy(fr["box3d"]), "scores": torch.from_numpy(fr["score"]),
                      "label_preds": torch.from_numpy(fr["label"])}
        path = os.path.join(root, "annos", tok)
        with open(path, "wb") as f:
            pickle.dump({"veh_to_global": fr["pose"]}, f)
        infos.append({"token": tok, "anno_path": path, "timestamp": fr["timestamp"]})
    infos = [infos[i] for i in np.random.default_rng(seed).permutation(len(infos))]
    return preds, infos


def run_tracker(tp, PubTracker, preds, infos, p):
    tracker = PubTracker(max_age=p["max_age"], max_dist={"VEHICLE": p["vehicle"], "PEDESTRIAN": p["pedestrian"],
                                                          "CYCLIST": p["cyclist"]}, score_thresh=p["score_thresh"])
    global_preds, _ = tp.convert_detection_to_global_box(preds, tp.reorganize_info(infos))
    out, cts, vels, toks = [], [], [], []
    for pred in global_preds:
        if pred["frame_id"] == 0:
            tracker.reset()
            last_time_stamp = pred["timestamp"]
        time_lag = pred["timestamp"] - last_time_stamp
        last_time_stamp = pred["timestamp"]
        dets = pred["global_boxs"]
        cts.append(np.array([d["translation"][:2] for d in dets], np.float64).reshape(-1, 2))
        vels.append(np.array([d["velocity"] for d in dets], np.float64).reshape(-1, 2))
        toks.append(pred["token"])
        outputs = tracker.step_centertrack(dets, time_lag)
        box_ids = [it["box_id"] for it in outputs if it["active"] != 0]
        tids = [it["tracking_id"] for it in outputs if it["active"] != 0]
        out.append((np.array(box_ids, np.int64), np.array(tids, np.int64)))
    return out, tracker.id_count, cts, vels, toks


def run_dense(PubTracker, inputs, max_age=3, max_dist=(0.8, 0.4, 0.6), score_thresh=0.75):
    """-> (per frame (box_ids, tracking_ids), id_count) of the reference's tracker on tracker-form inputs"""
    ct, tracking, label, score, fo, so = inputs
    names = ["VEHICLE", "PEDESTRIAN", "CYCLIST"]
    tracker = PubTracker(max_age=max_age, max_dist=dict(zip(names, max_dist)), score_thresh=score_thresh)
    starts = set(int(x) for x in so[:-1])
    out = []
    for f in range(len(fo) - 1):
        if f in starts:
            tracker.reset()
        dets = [{"translation": (ct[k, 0], ct[k, 1], 0.0), "velocity": -tracking[k], "detection_name": names[label[k]],
                 "score": float(score[k]), "box_id": k - int(fo[f])} for k in range(int(fo[f]), int(fo[f + 1]))]
        for d in dets:
            assert np.array_equal(np.array(d["velocity"][:2]) * -1 * 1.0, tracking[d["box_id"] + int(fo[f])])
        outputs = tracker.step_centertrack(dets, 1.0)
        keep = [it for it in outputs if it["active"] != 0]
        out.append((np.array([it["box_id"] for it in keep], np.int64), np.array([it["tracking_id"] for it in keep], np.int64)))
    return out, tracker.id_count


def write_npz(path, rec):
    """np.savez_compressed with fixed member dates, so that the file regenerates byte for byte"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in rec.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def dense(PubTracker, out_dir):
    rec = {}
    with np.errstate(invalid="ignore"):
        for name, (inputs, params) in track_ref.dense_cases().items():
            out, id_count = run_dense(PubTracker, inputs, **params)
            rec[name + "__box_ids"] = np.concatenate([o[0] for o in out] + [np.zeros(0, np.int64)]).astype(np.int32)
            rec[name + "__tracking_ids"] = np.concatenate([o[1] for o in out] + [np.zeros(0, np.int64)]).astype(np.int32)
            rec[name + "__out_count"] = np.array([len(o[0]) for o in out], np.int32)
            rec[name + "__id_count"] = np.array(id_count, np.int64)
            print(name, "frames", len(out), "entries", len(rec[name + "__box_ids"]), "ids", id_count)
    write_npz(os.path.join(out_dir, "tracking_dense.npz"), rec)


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    tp, PubTracker = import_test_py()
    dense(PubTracker, out_dir)
    frames = track_ref.scene(SEED)
    rec = {}
    with tempfile.TemporaryDirectory() as tmp:
        preds, infos = write_inputs(tmp, frames, SEED)
        out, id_count, cts, vels, toks = run_tracker(tp, PubTracker, preds, infos, PARAMS)
    assert toks == [fr["token"] for fr in frames], "track_ref.scene must list frames in sort_detections order"
    rec["box_ids"] = np.concatenate([o[0] for o in out])
    rec["tracking_ids"] = np.concatenate([o[1] for o in out])
    rec["out_count"] = np.array([len(o[0]) for o in out], np.int64)
    rec["id_count"] = np.array(id_count, np.int64)
    rec["ct"] = np.concatenate(cts)
    rec["velocity"] = np.concatenate(vels)
    # match: the tracked boxes in Waymo convention against each frame's annotation boxes
    boxes = np.concatenate([np.concatenate([fr["box3d"][:, :3], fr["box3d"][:, [4, 3, 5]],
                                            -fr["box3d"][:, 8:9] - np.float32(np.pi / 2)], axis=1) for fr in frames])
    offs = np.concatenate([[0], np.cumsum([len(fr["box3d"]) for fr in frames])])
    gts = [fr["gt"][:, [0, 1, 2, 3, 4, 5, -1]] for fr in frames]
    goff = np.concatenate([[0], np.cumsum([len(g) for g in gts])])
    gt = np.concatenate(gts)
    for f, (b, _) in enumerate(out):                    # the margin: no best IoU within 1e-5 of 0.75
        g = gt[goff[f]:goff[f + 1]]
        for k in b:
            box = boxes[offs[f] + k]
            if len(g) and np.isfinite(box).all():
                best = iou_ref.pairwise(box[None].astype(np.float64), g.astype(np.float64))[1][0].max()
                assert abs(best - 0.75) > 1e-5, (f, k, best)
    m = track_ref.match(out, boxes, offs, gt, goff, lambda a, b: iou_ref.pairwise(a, b)[1])
    flat = [x for row in m for x in row]
    rec["match_frame"] = np.array([-1 if x is None else x[0] for x in flat], np.int64)
    rec["match_obj"] = np.array([-1 if x is None else x[1] for x in flat], np.int64)
    # regroup: trackData.py on a val dir
    td = regroup_input(out, [fr["token"] for fr in frames])
    with tempfile.TemporaryDirectory() as tmp:
        wd = os.path.join(tmp, "val")
        os.makedirs(wd)
        with open(os.path.join(wd, "trackData.pkl"), "wb") as f:
            pickle.dump(td, f)
        sys.path.insert(0, os.path.join(REF, "tools"))
        import trackData
        argv = sys.argv
        sys.argv = ["trackData.py", "--work_dir", wd]
        try:
            trackData.main()
        finally:
            sys.argv = argv
        with open(os.path.join(wd, "track.pkl"), "rb") as f:
            tr = pickle.load(f)
    rec["regroup_ids"] = np.array(list(tr.keys()))
    rec["regroup_tokens"] = np.array(["|".join(v["token"]) for v in tr.values()])
    rec["regroup_scores"] = np.concatenate([np.asarray(v["score"], np.float64) for v in tr.values()])
    for k, v in rec.items():
        print(k, v.shape, v.dtype)
    print("matches:", int((rec["match_obj"] >= 0).sum()), "of", len(flat), "ids:", id_count)
    np.savez_compressed(os.path.join(out_dir, "tracking.npz"), **rec)


def regroup_input(out, tokens):
    """a trackData dict from the tracker's output (ids as strings; the other fields small stand-ins)"""
    td = {}
    for (b, t), tok in zip(out, tokens):
        td[tok] = {"id": [f"{int(x):032x}" for x in t], "type": [int(x) % 3 for x in b], "bbox": [np.full(7, float(x)) for x in b],
                   "score": [float(x) / 10 for x in b], "point": [np.zeros((int(x) % 3, 3)) for x in b],
                   "match": [None if x % 2 else f"m{x}" for x in b]}
    return td


if __name__ == "__main__":
    main()
