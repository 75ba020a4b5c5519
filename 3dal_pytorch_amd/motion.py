"""The motion-state run: tools/trackGT.py (the GT track table) and tools/motionState.py (track features, the linear SVM,
the static / dynamic split) with the grouping, the features and the classification on the device.

    python -m 3dal_pytorch_amd.motion gt --infos I --result R
    python -m 3dal_pytorch_amd.motion --track_train D --track_val D [--split 16] [--model PATH]

`gt` writes trackGT.pkl as trackGT.py does. The second form reads track_{i}.pkl + trackGT.pkl of the train dir and
track.pkl + trackGT.pkl of the val dir (track.py's `regroup` writes the first, `gt` the second), writes
trackStatic_{i}.pkl / trackDynamic_{i}.pkl in the train dir (split by the GT flag of the matched object), fits the SVM
on the train features, prints motionState.py's lines, writes trackStatic.pkl / trackDynamic.pkl in the val dir (split by
the prediction) and the model as motion_svm.json beside them. With --model the fit is skipped and that model classifies.

Resident path (no pickles, no host read-back until the caller asks):

    groups = group_tracks(result)                       # dal3_group_by_key over a track.TrackResult
    feats = track_features(groups, center, type, score, n_points, match)
    res = MotionResult(groups, feats, classify(feats.feature, feats.keep, model), result)
    res.kinds()  /  res.tracks(scores)                  # what track.segment_tracks takes / returns

Device work (csrc/dal3_motion.hip): dal3_group_by_key (a stable radix sort of (key, position) pairs: the regrouping of
trackData.py), dal3_track_features / dal3_gt_table (one pass over the groups, NumPy's float64 operation order),
dal3_motion_classify (the decision and the stable compaction into static and dynamic ids). Host work: the pickles, the
string-to-integer maps, the output dicts, and the SVM fit (fit_linear_svm: two features, a model of three numbers).

Deliberate departures from the reference:
- --split is parsed as int (motionState.py's untyped default breaks in range() when the flag is given);
- trackGT.pkl's 'vel' entries are computed in float64 on the device and stored in the dtype of obj['box'];
- no scikit-learn: fit_linear_svm solves the same soft-margin problem to a ten times tighter stop than libsvm's.
"""
import argparse
import json
import os
import pickle
import sys
import time

import numpy as np
import torch

from . import _hip


class bcolors:
    OKCYAN = "\033[96m"
    OKBLUE = "\033[94m"
    ENDC = "\033[0m"


# ------------------------------------------------------------------------------------------------ device calls
class Groups:
    """dal3_group_by_key's outputs, device tensors: group g = entry[group_start[g] : group_start[g + 1]] (input
    positions, ascending); n_groups (1) = the largest key + 1; status the device word (shared with a TrackResult)."""

    def __init__(self, group_start, entry, n_groups, status, T, E):
        self.group_start, self.entry, self.n_groups, self.status, self.T, self.E = group_start, entry, n_groups, status, T, E

    def check(self):
        """raise if the device reported a key outside [0, T) (a host sync)"""
        check_status(self.status)


def check_status(status):
    if int(status.item()) & _hip.MOTION_BAD_KEY:
        raise RuntimeError("motion: a key outside the group capacity, or a frame index outside the poses (status "
                           "DAL3_MOTION_BAD_KEY); its entries are in no group — run again with a larger capacity")


def group_by_key(keys, T, key_base=None, key_bias=0, frame_offsets=None, out_count=None, status=None, max_workgroups=0):
    """Stable grouping of keys (E) int64 on the device into T groups, one dal3_group_by_key call on the current stream,
    no host sync. key = keys[i] - key_base (optional device int64 (1)) - key_bias; frame_offsets (F+1) int64 /
    out_count (F) int32 as a TrackResult holds them restrict the entries to each frame's used slots. status: an
    existing device status word to OR into (else a fresh one)."""
    dev = keys.device
    E, T = int(keys.numel()), int(T)
    F = int(out_count.numel()) if out_count is not None else 0
    lib = _hip.lib()
    ws = _hip.workspace(lib.dal3_group_workspace_bytes(E, T), dev)
    group_start = torch.empty(T + 1, dtype=torch.int64, device=dev)
    entry = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    n_groups = torch.empty(1, dtype=torch.int64, device=dev)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    a = _hip.GroupArgs()
    a.E, a.T, a.F = E, T, F
    a.keys, a.key_base, a.key_bias = _hip.ptr(keys), _hip.ptr(key_base), int(key_bias)
    a.frame_offsets, a.out_count = _hip.ptr(frame_offsets), _hip.ptr(out_count)
    a.group_start, a.entry, a.n_groups, a.status = _hip.ptr(group_start), _hip.ptr(entry), _hip.ptr(n_groups), _hip.ptr(status)
    a.max_workgroups, a.workspace, a.workspace_bytes = int(max_workgroups), _hip.ptr(ws), ws.numel()
    _hip.check(lib.dal3_group_by_key(a, _hip.stream()))
    return Groups(group_start, entry[:E], n_groups, status, T, E)


def group_tracks(result, capacity=None, max_workgroups=0):
    """the device CSR of a track.TrackResult: group g = the output positions of tracking id id_base + 1 + g, in frame
    order. capacity: the number of ids to make room for (default: one per detection slot, which always suffices).
    No host sync; a bad id lands in result.status (check())."""
    E = int(result.tracking_ids.numel()) if result.frame_offsets.numel() > 1 else 0
    keys = result.tracking_ids[:E] if E else result.tracking_ids[:0]
    T = int(capacity) if capacity else E
    F = int(result.out_count.numel())
    return group_by_key(keys, T, result.id_base, 1, result.frame_offsets if F else None, result.out_count if F else None,
                        result.status, max_workgroups)


def detection_index(result):
    """(E) int64 device tensor: the detection (row of the flat per-detection arrays, frames in order) at each output
    position of a TrackResult, for gathering per-detection arrays into per-entry ones. Positions past a frame's
    out_count are no entries: they get an arbitrary valid row. No host sync."""
    E = int(result.tracking_ids.numel())
    off = result.frame_offsets
    pos = torch.arange(E, dtype=torch.int64, device=off.device)
    f = (torch.searchsorted(off, pos, right=True) - 1).clamp_(0, max(int(off.numel()) - 2, 0))
    return (off[f] + result.box_ids[:E].to(torch.int64)).clamp_(0, max(E - 1, 0))


class Features:
    """dal3_track_features' outputs per group (device tensors)"""

    def __init__(self, n, type0, match_last, points_sum, best, keep, feature):
        self.n, self.type0, self.match_last, self.points_sum = n, type0, match_last, points_sum
        self.best, self.keep, self.feature = best, keep, feature


def track_features(groups, center, type, score, n_points, match, max_workgroups=0):
    """trackFeature (motionState.py:30-67) per group. Per-entry device arrays by input position: center (E,3) float64
    (global frame), type (E) int32, score (E) float32, n_points (E) int32, match (E) int32 (GT object index, -1 None).
    No host sync."""
    dev = groups.group_start.device
    T, E = groups.T, groups.E
    for name, t, dt in (("center", center, torch.float64), ("type", type, torch.int32), ("score", score, torch.float32),
                        ("n_points", n_points, torch.int32), ("match", match, torch.int32)):
        if t.dtype != dt or not t.is_contiguous() or t.shape[0] < E:
            raise ValueError(f"track_features: {name} must be a contiguous {dt} tensor with a row per entry")
    n = max(T, 1)
    out = Features(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev),
                   torch.empty((n, 2), dtype=torch.float64, device=dev))
    a = _hip.TrackFeatureArgs()
    a.T, a.E = T, E
    a.group_start, a.entry, a.n_groups = _hip.ptr(groups.group_start), _hip.ptr(groups.entry), _hip.ptr(groups.n_groups)
    a.center, a.type, a.score, a.n_points, a.match = (_hip.ptr(center), _hip.ptr(type), _hip.ptr(score), _hip.ptr(n_points),
                                                      _hip.ptr(match))
    a.n, a.type0, a.match_last, a.points_sum = _hip.ptr(out.n), _hip.ptr(out.type0), _hip.ptr(out.match_last), _hip.ptr(out.points_sum)
    a.best, a.keep, a.feature, a.max_workgroups = _hip.ptr(out.best), _hip.ptr(out.keep), _hip.ptr(out.feature), int(max_workgroups)
    _hip.check(_hip.lib().dal3_track_features(a, _hip.stream()))
    for k in ("n", "type0", "match_last", "points_sum", "best", "keep", "feature"):
        setattr(out, k, getattr(out, k)[:T])
    return out


class GtTable:
    """dal3_gt_table's outputs: per entry box_global (E,7), vel (E); per object n, dist, max_vel, is_static"""

    def __init__(self, box_global, vel, n, dist, max_vel, is_static):
        self.box_global, self.vel, self.n, self.dist, self.max_vel, self.is_static = box_global, vel, n, dist, max_vel, is_static


def gt_table(groups, box, frame, pose, max_workgroups=0):
    """trackGT.py:43-66 on the device: box (E,9) float64 annotation rows (vehicle frame), frame (E) int32, pose (F,16)
    float64 veh_to_global; groups keyed by GT object. A bad frame index lands in groups.status. No host sync."""
    dev = groups.group_start.device
    T, E, F = groups.T, groups.E, int(pose.shape[0])
    if box.dtype != torch.float64 or frame.dtype != torch.int32 or pose.dtype != torch.float64:
        raise ValueError("gt_table: box / pose float64, frame int32")
    out = GtTable(torch.empty((max(E, 1), 7), dtype=torch.float64, device=dev), torch.empty(max(E, 1), dtype=torch.float64, device=dev),
                  torch.empty(max(T, 1), dtype=torch.int32, device=dev), torch.empty(max(T, 1), dtype=torch.float64, device=dev),
                  torch.empty(max(T, 1), dtype=torch.float64, device=dev), torch.empty(max(T, 1), dtype=torch.uint8, device=dev))
    a = _hip.GtTableArgs()
    a.T, a.E, a.F = T, E, F
    a.group_start, a.entry = _hip.ptr(groups.group_start), _hip.ptr(groups.entry)
    a.box, a.frame, a.pose = _hip.ptr(box.contiguous()), _hip.ptr(frame.contiguous()), _hip.ptr(pose.contiguous())
    a.box_global, a.vel, a.n, a.dist = _hip.ptr(out.box_global), _hip.ptr(out.vel), _hip.ptr(out.n), _hip.ptr(out.dist)
    a.max_vel, a.is_static, a.status, a.max_workgroups = _hip.ptr(out.max_vel), _hip.ptr(out.is_static), _hip.ptr(groups.status), int(max_workgroups)
    _hip.check(_hip.lib().dal3_gt_table(a, _hip.stream()))
    out.box_global, out.vel = out.box_global[:E], out.vel[:E]
    out.n, out.dist, out.max_vel, out.is_static = out.n[:T], out.dist[:T], out.max_vel[:T], out.is_static[:T]
    return out


class Classes:
    """dal3_motion_classify's outputs: decision (T) float64, is_static (T) uint8, static_ids / dynamic_ids (T) int32 of
    which the first counts[0] / counts[1] are set (ascending group index), counts (2) int64 on the device"""

    def __init__(self, decision, is_static, static_ids, dynamic_ids, counts):
        self.decision, self.is_static, self.static_ids, self.dynamic_ids, self.counts = decision, is_static, static_ids, dynamic_ids, counts

    def ids(self):
        """(static ids, dynamic ids) as NumPy arrays (a download)"""
        c = self.counts.cpu().numpy()
        return self.static_ids.cpu().numpy()[:c[0]], self.dynamic_ids.cpu().numpy()[:c[1]]


def classify(features, keep, model, max_workgroups=0):
    """decision = features . w + b in float64, static = decision > 0 (SVC's binary rule: positive -> classes_[1] = 1 =
    static), kept groups compacted in order. features (T,2) float64 / keep (T) uint8 device tensors; model = (w, b)
    host numbers. No host sync."""
    dev = features.device
    T = int(features.shape[0])
    w, b = model
    lib = _hip.lib()
    ws = _hip.workspace(lib.dal3_motion_classify_workspace_bytes(T), dev)
    n = max(T, 1)
    out = Classes(torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev),
                  torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                  torch.empty(2, dtype=torch.int64, device=dev))
    a = _hip.MotionClassifyArgs()
    a.T, a.feature, a.keep = T, _hip.ptr(features), _hip.ptr(keep)
    a.w[0], a.w[1], a.b = float(w[0]), float(w[1]), float(b)
    a.decision, a.is_static, a.static_ids, a.dynamic_ids = (_hip.ptr(out.decision), _hip.ptr(out.is_static), _hip.ptr(out.static_ids),
                                                            _hip.ptr(out.dynamic_ids))
    a.counts, a.max_workgroups, a.workspace, a.workspace_bytes = _hip.ptr(out.counts), int(max_workgroups), _hip.ptr(ws), ws.numel()
    _hip.check(lib.dal3_motion_classify(a, _hip.stream()))
    out.decision, out.is_static = out.decision[:T], out.is_static[:T]
    return out


class MotionResult:
    """groups + features + classes of one run; with the TrackResult the groups came from, kinds() and tracks() speak
    in tracking ids and (frame, detection) pairs"""

    def __init__(self, groups, features, classes, result=None):
        self.groups, self.features, self.classes, self.result = groups, features, classes, result

    def check(self):
        """raise if the device reported a problem (a host sync)"""
        if self.result is not None:
            self.result.check()
        self.groups.check()

    def _id0(self):
        """the id of group 0"""
        if self.result is None:
            return 0
        return (int(self.result.id_base.item()) if self.result.id_base is not None else 0) + 1

    def kinds(self):
        """{id: "static" | "dynamic"} of the kept groups, ascending id — what track.segment_tracks takes"""
        self.check()
        s, d = self.classes.ids()
        ids = np.concatenate([s, d]).astype(np.int64)
        kind = np.concatenate([np.ones(len(s), bool), np.zeros(len(d), bool)])
        order = np.argsort(ids, kind="stable")
        id0 = self._id0()
        return {int(g) + id0: ("static" if st else "dynamic") for g, st in zip(ids[order].tolist(), kind[order].tolist())}

    def tracks(self, scores, frame_range=None):
        """segment.SegmentPlan's `tracks` — equal to track.segment_tracks(frames, self.kinds(), scores) — from the CSR,
        one slice per track. scores: per frame the detections' scores. frame_range (lo, hi): the segment's frames of
        the result (scores for those frames only; frame numbers count from lo); default every frame."""
        if self.result is None:
            raise ValueError("tracks() needs the TrackResult the groups were made from")
        kinds = self.kinds()
        gs, entry = self.groups.group_start.cpu().numpy(), self.groups.entry.cpu().numpy().astype(np.int64)
        off = self.result.frame_offsets.cpu().numpy()
        lo, hi = frame_range if frame_range is not None else (0, len(off) - 1)
        entry = entry[:gs[-1]]
        frame = np.searchsorted(off, entry, side="right") - 1
        k = self.result.box_ids.cpu().numpy().astype(np.int64)[entry]
        flat = np.concatenate([np.asarray(s).reshape(-1) for s in scores]) if len(scores) else np.zeros(0, np.float32)
        inside = (frame >= lo) & (frame < hi)
        sc = np.zeros(len(entry), flat.dtype)
        sc[inside] = flat[off[frame[inside]] - off[lo] + k[inside]]
        frame = frame - lo
        id0, out = self._id0(), []
        for tid, kind in kinds.items():
            a, b = gs[tid - id0], gs[tid - id0 + 1]
            a, b = a + np.searchsorted(entry[a:b], off[lo]), a + np.searchsorted(entry[a:b], off[hi])
            if b > a:
                out.append((entry[a], {"kind": kind, "dets": list(zip(frame[a:b].tolist(), k[a:b].tolist())), "score": list(sc[a:b]),
                                       "id": tid}))
        out.sort(key=lambda t: t[0])                        # order of first appearance (inside the frame range)
        return [t for _, t in out]


def motion_state(result, center, type, score, n_points, match, model, capacity=None, max_workgroups=0):
    """group -> features -> classify for a TrackResult; per-entry arrays by output position (as dal3_track_match's
    outputs are). capacity: the number of ids to make room for (default: one per detection slot). None of the three
    calls reads back: no host sync."""
    groups = group_tracks(result, capacity, max_workgroups)
    feats = track_features(groups, center, type, score, n_points, match, max_workgroups)
    return MotionResult(groups, feats, classify(feats.feature, feats.keep, model, max_workgroups), result)


# ------------------------------------------------------------------------------------------------ the SVM (host)
def fit_linear_svm(X, y, C=1.0, tol=1e-4, max_iter=10_000_000, info=None):
    """The soft-margin linear SVM of SVC(kernel='linear', C): min 1/2 |w|^2 + C sum hinge(y_i (w.x_i + b)), bias not
    regularised, solved in the dual by SMO with libsvm's second-order working-set selection and shrinking, float64 NumPy.
    The kernel is linear, so w = sum alpha_i y_i x_i is kept explicitly: a step updates the gradient of the active set
    with one matrix-vector product, and the gradient of a shrunk variable is rebuilt from w when it is needed again.
    Stops when the maximal KKT violation m(alpha) - M(alpha) over ALL variables is below tol (libsvm's default is
    1e-3). y: labels 0 / 1 (1 = static = the positive class). Returns (w (2,), b); info: an optional dict that receives
    alpha, the final violation, the iterations and the seconds taken."""
    t0 = time.perf_counter()
    X = np.ascontiguousarray(X, np.float64)
    y01 = np.asarray(y).reshape(-1)
    N = X.shape[0]
    if N == 0 or len(np.unique(y01)) < 2:
        raise ValueError("fit_linear_svm: needs samples of both classes")
    ys = np.where(y01 > 0, 1.0, -1.0)
    C = float(C)
    alpha = np.zeros(N)
    w = np.zeros(X.shape[1])
    sq = np.einsum("ij,ij->i", X, X)
    tau = 1e-12

    def violation(G, yy, al):
        v = -yy * G
        up = ((yy > 0) & (al < C)) | ((yy < 0) & (al > 0))
        low = ((yy > 0) & (al > 0)) | ((yy < 0) & (al < C))
        return v, up, low

    active = np.arange(N)
    Xa, ya, sqa = X, ys, sq
    Ga = -np.ones(N)                                        # G = Q alpha - e at alpha = 0
    it, since_shrink, shrink_every = 0, 0, min(N, 1000)
    while it < max_iter:
        al = alpha[active]
        v, up, low = violation(Ga, ya, al)
        gmax = v[up].max() if up.any() else -np.inf
        gmin = v[low].min() if low.any() else np.inf
        if gmax - gmin < tol:
            if len(active) == N:
                break
            # converged on the active set: every gradient again from w, every variable active
            active = np.arange(N)
            Xa, ya, sqa = X, ys, sq
            w = X.T @ (alpha * ys)
            Ga = ys * (X @ w) - 1.0
            since_shrink = 0
            continue
        i = int(np.argmax(np.where(up, v, -np.inf)))
        # second order: among the violating t in I_low, the largest decrease -(b_t^2) / a_t
        bt = gmax - v
        at = sqa[i] + sqa - 2.0 * (Xa @ Xa[i])
        at = np.where(at > 0, at, tau)
        cand = low & (bt > 0)
        j = int(np.argmax(np.where(cand, bt * bt / at, -np.inf)))
        room_i = C - al[i] if ya[i] > 0 else al[i]          # how far alpha_i += y_i lam and alpha_j -= y_j lam may go
        room_j = al[j] if ya[j] > 0 else C - al[j]
        lam = min(bt[j] / at[j], room_i, room_j)
        # a variable that reaches its bound is set to the bound itself, so that the index sets stay exact
        alpha[active[i]] = (C if ya[i] > 0 else 0.0) if lam == room_i else al[i] + ya[i] * lam
        alpha[active[j]] = (0.0 if ya[j] > 0 else C) if lam == room_j else al[j] - ya[j] * lam
        dw = lam * (Xa[i] - Xa[j])
        w = w + dw
        Ga = Ga + ya * (Xa @ dw)
        it += 1
        since_shrink += 1
        if since_shrink >= shrink_every:
            since_shrink = 0
            al = alpha[active]
            v, up, low = violation(Ga, ya, al)
            gmax = v[up].max() if up.any() else -np.inf
            gmin = v[low].min() if low.any() else np.inf
            if gmax - gmin > tol:
                # a variable at a bound that no pair can move: only in I_low and above every I_up value, or the reverse
                out = (~up & (v > gmax)) | (~low & (v < gmin))
                if out.any() and not out.all():
                    keep = ~out
                    active, Xa, ya, sqa, Ga = active[keep], Xa[keep], ya[keep], sqa[keep], Ga[keep]
    else:
        raise RuntimeError("fit_linear_svm: no convergence")
    # the gradients once more from the final alpha, and the bias as libsvm forms rho: the mean of y G over the free
    # variables, else the middle of the bounds
    w = X.T @ (alpha * ys)
    G = ys * (X @ w) - 1.0
    v, up, low = violation(G, ys, alpha)
    free = (alpha > 0) & (alpha < C)
    if free.any():
        b = float(np.mean(v[free]))
    else:
        b = float((v[up].max() + v[low].min()) / 2.0)
    if info is not None:
        info.update(alpha=alpha, violation=float(v[up].max() - v[low].min()), iterations=it, seconds=time.perf_counter() - t0)
    return w, b


def save_model(path, w, b):
    with open(path, "w") as f:
        json.dump({"w": [float(w[0]), float(w[1])], "b": float(b)}, f)


def load_model(path):
    with open(path) as f:
        m = json.load(f)
    return np.asarray(m["w"], np.float64), float(m["b"])


# ------------------------------------------------------------------------------------------------ file level
def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _dump(obj, path):
    with open(path, "wb") as f:
        pickle.dump(obj, f)


def build_gt(infos, device="cuda"):
    """trackGT.py:main's table from the infos list: names -> integer keys on the host (first appearance = the
    reference's dict order), the transforms and the per-object reductions on the device."""
    dev = torch.device(device)
    key_of, names, first_pose = {}, [], []
    keys, rows, frame, num_points, poses = [], [], [], [], []
    dtype = np.float64
    for f, info in enumerate(infos):
        annos = _load(info["anno_path"])
        pose = np.reshape(annos["veh_to_global"], [4, 4])
        poses.append(np.asarray(pose, np.float64).reshape(16))
        for obj in annos["objects"]:
            name = obj["name"]
            k = key_of.get(name)
            if k is None:
                k = key_of[name] = len(names)
                names.append(name)
                first_pose.append(pose)
            box = np.array(obj["box"])
            dtype = box.dtype
            keys.append(k)
            rows.append(box.astype(np.float64))
            frame.append(f)
            num_points.append(obj["num_points"])
    T, E = len(names), len(keys)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731
    groups = group_by_key(t(np.asarray(keys, np.int64), np.int64), T)
    table = gt_table(groups, t(np.asarray(rows, np.float64).reshape(E, 9), np.float64), t(np.asarray(frame), np.int32),
                     t(np.asarray(poses, np.float64).reshape(len(poses), 16), np.float64))
    groups.check()
    gs, entry = groups.group_start.cpu().numpy(), groups.entry.cpu().numpy()
    box_g, vel, static = table.box_global.cpu().numpy(), table.vel.cpu().numpy().astype(dtype), table.is_static.cpu().numpy()
    out = {}
    for k, name in enumerate(names):
        e = entry[gs[k]:gs[k + 1]]
        out[name] = {"box": list(box_g[e]), "vel": list(vel[e]), "pose": first_pose[k],
                     "num_points": [num_points[i] for i in e], "static": int(static[k])}
    return out


def run_gt(infos_path, result_path, device="cuda"):
    track_gt = build_gt(_load(infos_path), device)
    _dump(track_gt, result_path)
    return track_gt


def flatten_tracks(track, track_gt):
    """{track id: obj} in dict order -> the per-entry arrays (keys = position of the track, match = row of trackGT.pkl)"""
    gt_row = {name: r for r, name in enumerate(track_gt.keys())}
    lens = np.asarray([len(o["bbox"]) for o in track.values()], np.int64)
    keys = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    E = int(lens.sum())
    bbox = np.asarray([b for o in track.values() for b in o["bbox"]], np.float64).reshape(E, -1)
    match = np.asarray([-1 if m is None else gt_row[m] for o in track.values() for m in o["match"]], np.int32)
    return {"keys": keys, "center": np.ascontiguousarray(bbox[:, :3]),
            "type": np.asarray([x for o in track.values() for x in o["type"]], np.int32),
            "score": np.asarray([x for o in track.values() for x in o["score"]], np.float32),
            "n_points": np.asarray([len(p) for o in track.values() for p in o["point"]], np.int32), "match": match}


def features_of(track, track_gt, device="cuda"):
    """trackFeature's table for a track dict on the device -> (Groups, Features); a download is the caller's"""
    dev = torch.device(device)
    flat = flatten_tracks(track, track_gt)
    t = {k: torch.from_numpy(v).to(dev) for k, v in flat.items()}
    groups = group_by_key(t["keys"], len(track))
    feats = track_features(groups, t["center"], t["type"], t["score"], t["n_points"], t["match"])
    return groups, feats


def run(track_train, track_val, split=16, model_path=None, device="cuda"):
    """motionState.py:main. Returns (w, b)."""
    c, e = bcolors.OKCYAN, bcolors.ENDC
    gt_static = lambda gt: np.asarray([int(o["static"]) for o in gt.values()], np.int64)   # noqa: E731
    print(f"{c}>{e} Reading train data")
    train = {}
    for i in range(split):
        train.update(_load(os.path.join(track_train, f"track_{i}.pkl")))
    print(f"{c}>{e} Reading train GT data")
    gt_train = _load(os.path.join(track_train, "trackGT.pkl"))
    print(f"{c}>{e} Processing train data")
    groups, feats = features_of(train, gt_train, device)
    groups.check()
    keep = feats.keep.cpu().numpy().astype(bool)
    trainX = feats.feature.cpu().numpy()[keep]
    trainY = (gt_static(gt_train)[feats.match_last.cpu().numpy()[keep]] != 0).astype(np.int64)
    items = [it for it, k in zip(train.items(), keep) if k]
    static_list = [it for it, yv in zip(items, trainY) if yv == 1]
    dynamic_list = [it for it, yv in zip(items, trainY) if yv == 0]
    del train
    for name, lst, label in (("trackStatic", static_list, "trackStatic.pkl"), ("trackDynamic", dynamic_list, "trackDynamic.pkl")):
        print(f"{c}>{e} Saving train/{label}")
        for i in range(split):
            _dump(dict(lst[len(lst) * i // split:len(lst) * (i + 1) // split]), os.path.join(track_train, f"{name}_{i}.pkl"))
    print(f"{c}>{e} Reading val data")
    val = _load(os.path.join(track_val, "track.pkl"))
    print(f"{c}>{e} Reading val GT data")
    gt_val = _load(os.path.join(track_val, "trackGT.pkl"))
    print(f"{c}>{e} Processing val data")
    vgroups, vfeats = features_of(val, gt_val, device)
    vgroups.check()
    vkeep = vfeats.keep.cpu().numpy().astype(bool)
    valY = (gt_static(gt_val)[vfeats.match_last.cpu().numpy()[vkeep]] != 0).astype(np.int64)
    print(f"[{bcolors.OKBLUE}Info{e}] Number of train: {trainX.shape[0]}")
    print(f"[{bcolors.OKBLUE}Info{e}] Number of val: {int(vkeep.sum())}")
    if model_path:
        w, b = load_model(model_path)
    else:
        w, b = fit_linear_svm(trainX, trainY)
    cls = classify(vfeats.feature, vfeats.keep, (w, b))
    s_ids, d_ids = cls.ids()
    pred = cls.is_static.cpu().numpy()[vkeep].astype(np.int64)
    print(f"{c}>{e} Score on test set: {float(np.mean(pred == valY)) if len(valY) else float('nan')}")
    vitems = list(val.items())
    print(f"{c}>{e} Saving val/trackStatic.pkl")
    _dump({vitems[g][0]: vitems[g][1] for g in s_ids}, os.path.join(track_val, "trackStatic.pkl"))
    print(f"{c}>{e} Saving val/trackDynamic.pkl")
    _dump({vitems[g][0]: vitems[g][1] for g in d_ids}, os.path.join(track_val, "trackDynamic.pkl"))
    save_model(os.path.join(track_val, "motion_svm.json"), w, b)
    return w, b


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if argv and argv[0] == "gt":
        p = argparse.ArgumentParser(prog="3dal_pytorch_amd.motion gt")
        p.add_argument("--infos", help="Path to infos file.")
        p.add_argument("--result", help="Path to result file.")
        args = p.parse_args(argv[1:])
        run_gt(args.infos, args.result)
        return
    p = argparse.ArgumentParser(prog="3dal_pytorch_amd.motion")
    p.add_argument("--track_train", help="Path to train track data.")
    p.add_argument("--track_val", help="Path to val track data.")
    p.add_argument("--split", type=int, default=16, help="Number of train split.")
    p.add_argument("--model", default=None, help="motion_svm.json of an earlier run: classify without fitting.")
    args = p.parse_args(argv)
    run(args.track_train, args.track_val, args.split, args.model)


if __name__ == "__main__":
    main()
