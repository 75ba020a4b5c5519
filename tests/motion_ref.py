"""NumPy restatement of the motion-state run (include/dal3.h, dal3_group_by_key / dal3_track_features / dal3_gt_table /
dal3_motion_classify): test infrastructure, the oracle the kernels are held to, and the seeded work dirs
tests/golden/motion.npz was recorded on (tests/golden/gen_motion.py runs the reference's tools/trackGT.py and
tools/motionState.py on them).
"""
import os
import pickle

import numpy as np


# ---------------------------------------------------------------------------------------------- restatement
def group(keys, T):
    """-> (group_start (T+1) int64, entry int32): the stable counting sort, keys outside [0, T) left out"""
    keys = np.asarray(keys, np.int64)
    ok = (keys >= 0) & (keys < T)
    pos = np.nonzero(ok)[0]
    order = pos[np.argsort(keys[pos], kind="stable")]
    start = np.concatenate([[0], np.cumsum(np.bincount(keys[pos], minlength=T))]).astype(np.int64)
    return start, order.astype(np.int32)


def features(start, entry, center, type_, score, n_points, match):
    """dal3_track_features per group with NumPy's own calls (trackFeature, motionState.py:30-67)"""
    T = len(start) - 1
    out = {"n": np.zeros(T, np.int32), "type0": np.zeros(T, np.int32), "match_last": np.full(T, -1, np.int32),
           "points_sum": np.zeros(T, np.int64), "best": np.zeros(T, np.int32), "keep": np.zeros(T, np.uint8),
           "feature": np.zeros((T, 2))}
    for g in range(T):
        e = entry[start[g]:start[g + 1]]
        n = len(e)
        out["n"][g] = n
        if n == 0:
            continue
        c = center[e]
        out["type0"][g], out["match_last"][g] = type_[e[0]], match[e[-1]]
        out["points_sum"][g] = n_points[e].sum()
        out["best"][g] = np.argmax(score[e])
        out["keep"][g] = not (match[e[-1]] < 0 or n < 7 or type_[e[0]] == 2 or n_points[e].sum() == 0)
        out["feature"][g] = [np.linalg.norm(c[0] - c[-1]), np.linalg.norm(np.var(c, axis=0))]
    return out


def track_feature(track, track_gt):
    """trackFeature(track, trackGT) -> (X, Y, kept ids), the reference's expressions on its own dicts"""
    X, Y, ids = [], [], []
    for tid, obj in track.items():
        match = obj["match"][-1]
        bbox = np.array(obj["bbox"])
        if match is None or bbox.shape[0] < 7 or np.array(obj["type"])[0] == 2 or np.vstack(obj["point"]).shape[0] == 0:
            continue
        X.append([np.linalg.norm(bbox[0, :3] - bbox[-1, :3]), np.linalg.norm(np.var(bbox[:, :3], axis=0))])
        Y.append(0 if int(track_gt[match]["static"]) == 0 else 1)
        ids.append(tid)
    return np.array(X), np.array(Y), ids


def transform_box(box, pose):
    """trackGT.py:12-25"""
    heading = box[..., -1] + np.arctan2(pose[..., 1, 0], pose[..., 0, 0])
    center = np.einsum("...ij,...nj->...ni", pose[..., 0:3, 0:3], box[..., 0:3]) + np.expand_dims(pose[..., 0:3, 3], axis=-2)
    return np.squeeze(np.concatenate([center, box[..., 3:6], heading[..., np.newaxis]], axis=-1))


def gt_table(frames):
    """trackGT.py:36-66 on the scene's frames -> the trackGT dict"""
    gt = {}
    for fr in frames:
        pose = np.reshape(fr["pose"], [4, 4])
        for obj in fr["objects"]:
            box = transform_box(np.array(obj["box"])[[0, 1, 2, 3, 4, 5, -1]][np.newaxis, ...], pose)
            vel = np.linalg.norm(np.array(obj["box"])[[6, 7]])
            rec = gt.setdefault(obj["name"], {"box": [], "vel": [], "pose": pose, "num_points": []})
            rec["box"].append(box)
            rec["vel"].append(vel)
            rec["num_points"].append(obj["num_points"])
    for rec in gt.values():
        bbox = np.array(rec["box"])
        rec["static"] = 1 if np.linalg.norm(bbox[0, :3] - bbox[-1, :3]) < 1 and np.max(rec["vel"]) < 1 else 0
    return gt


# ---------------------------------------------------------------------------------------------- seeded inputs
def scene(seed, n_seq, n_frames=30, n_obj=30, dt=0.1, id0=1):
    """One work dir's content: (frames, tracks). frames: per frame token / pose (flat-16 veh_to_global) / objects
    [{name, box (9,) float32 in the vehicle frame, num_points}]; tracks: {id: type / bbox / score / point / match / token
    lists} as track.pkl holds them. Global coordinates are of the order 10^4 m. Planted: parked objects seen with
    centimetre jitter, movers from 0 to 12 m/s (the slow ones are static by the GT rule, so the classes overlap),
    pedestrians, tracks shorter than 7, tracks never matched, tracks matched late, tracks without a point."""
    rng = np.random.default_rng(seed)
    frames, tracks, tid = [], {}, id0
    for s in range(n_seq):
        a0 = rng.uniform(-np.pi, np.pi)
        base = rng.uniform(-2e4, 2e4, 3) * [1, 1, 0.01]
        poses = []
        for f in range(n_frames):
            a = a0 + 0.01 * f
            m = np.eye(4)
            m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
            m[:3, 3] = base + [np.cos(a0) * 1.0 * f, np.sin(a0) * 1.0 * f, 0.0]
            poses.append(m)
        objs = [[] for _ in range(n_frames)]
        for o in range(n_obj):
            name = f"gt{seed}_{s}_{o}"
            u = rng.uniform()
            kind = 1 if u < 0.4 else (2 if u < 0.85 else 3)          # parked, mover, pedestrian
            typ = 2 if kind == 3 else int(rng.choice([1, 4]))
            speed = 0.0 if kind == 1 else (rng.uniform(0, 12) if kind == 2 else rng.uniform(0, 2))
            th = rng.uniform(-np.pi, np.pi)
            p0 = poses[0][:3, 3] + np.append(rng.uniform(-50, 50, 2), rng.uniform(-1, 1))
            size = rng.uniform(0.5, 5, 3)
            lo = int(rng.integers(0, n_frames - 3))
            hi = int(rng.integers(lo + 3, n_frames + 1))
            centres = {}
            for f in range(lo, hi):
                pg = p0 + speed * dt * f * np.array([np.cos(th), np.sin(th), 0.0])
                centres[f] = pg
                R, t = poses[f][:3, :3], poses[f][:3, 3]
                pv = R.T @ (pg - t)
                vg = speed * np.array([np.cos(th), np.sin(th), 0.0]) + (rng.normal(0, 0.01, 3) if kind == 1 else 0)
                vv = R.T @ vg
                box = np.array([*pv, *size, vv[0], vv[1], th - (a0 + 0.01 * f)], np.float32)
                objs[f].append({"name": name, "box": box, "num_points": int(rng.integers(0, 200))})
            # the object's track: a part of its life, detections around the GT centre
            t_lo = int(rng.integers(lo, hi))
            t_hi = int(rng.integers(t_lo + 1, hi + 1))
            if rng.uniform() < 0.7:
                t_lo, t_hi = lo, hi
            n = t_hi - t_lo
            unmatched = rng.uniform() < 0.1
            late = int(rng.integers(0, 3))
            empty = rng.uniform() < 0.07
            sigma = 0.02 if kind == 1 else 0.1
            rec = {"type": [], "bbox": [], "score": [], "point": [], "match": [], "token": []}
            for r, f in enumerate(range(t_lo, t_hi)):
                c = centres[f] + rng.normal(0, sigma, 3)
                rec["type"].append(typ)
                rec["bbox"].append(np.array([*c, *size, th], np.float64))
                rec["score"].append(np.float32(rng.uniform(0.3, 1.0)))
                rec["point"].append(np.zeros((0, 3)) if empty else rng.normal(0, 1, (int(rng.integers(0, 4)), 3)) + c)
                rec["match"].append(None if unmatched or (r < late and r < n - 1) else name)
                rec["token"].append(f"seq_{s}_frame_{f}.pkl")
            tracks[f"{tid:032x}"] = rec
            tid += 1
        for f in range(n_frames):
            frames.append({"token": f"seq_{s}_frame_{f}.pkl", "pose": poses[f].reshape(16), "objects": objs[f]})
    return frames, tracks


TRAIN = dict(seed=4101, n_seq=40)
VAL = dict(seed=4102, n_seq=15, id0=100001)
SPLIT = 16


def write_dir(root, name, frames, tracks, split=None):
    """the files trackGT.py and motionState.py read: annos + infos, and track.pkl or track_{i}.pkl"""
    wd = os.path.join(root, name)
    os.makedirs(os.path.join(wd, "annos"), exist_ok=True)
    infos = []
    for fr in frames:
        path = os.path.join(wd, "annos", fr["token"])
        with open(path, "wb") as f:
            pickle.dump({"veh_to_global": fr["pose"], "objects": fr["objects"]}, f)
        infos.append({"token": fr["token"], "anno_path": path})
    with open(os.path.join(wd, "infos.pkl"), "wb") as f:
        pickle.dump(infos, f)
    if split:
        items = list(tracks.items())
        for i in range(split):
            with open(os.path.join(wd, f"track_{i}.pkl"), "wb") as f:
                pickle.dump(dict(items[len(items) * i // split:len(items) * (i + 1) // split]), f)
    else:
        with open(os.path.join(wd, "track.pkl"), "wb") as f:
            pickle.dump(tracks, f)
    return wd


def write_work_dirs(root):
    """-> (train dir, val dir, (train frames, train tracks), (val frames, val tracks))"""
    tr, va = scene(**TRAIN), scene(**VAL)
    return write_dir(root, "train", *tr, split=SPLIT), write_dir(root, "val", *va), tr, va


def big_keys(seed, E=5_300_000, T=400_000):
    """-> (keys (E) int64 in [0, T), T, ids of empty groups, the id of a one-entry group, the id of a 198-entry group)"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, T, E).astype(np.int64)
    special = rng.choice(T, 2000, replace=False)            # emptied; two of them refilled below
    fill = int(np.setdiff1d(np.arange(T), special)[0])
    keys[np.isin(keys, special)] = fill
    single, long = int(special[0]), int(special[1])
    where = rng.choice(E, 199, replace=False)
    keys[where[0]] = single
    keys[where[1:]] = long
    return keys, T, special[2:], single, long
