"""The baseline runs: the tracker's OWN boxes scored against ground truth on the device — what the numbers of
`python -m 3dal_pytorch_amd.eval` are read against. The reference's tools/static_init.py, tools/dynamic_init.py and
tools/eval.py with their per-(track, frame) Python loops replaced by flat tables and two kernels of lib3dal_hip.so
(dal3_score_tracks, dal3_best_gt_iou; include/dal3.h):

    python -m 3dal_pytorch_amd.baseline static  --track trackStatic.pkl  --infos infos.pkl --det_annos det_annos.pkl
    python -m 3dal_pytorch_amd.baseline dynamic --track trackDynamic.pkl --infos infos.pkl
    python -m 3dal_pytorch_amd.baseline labels  --track trackStatic.pkl  --infos infos.pkl --static static_labels.pkl

static   `[Init]` lines (every track-frame's own box against its ground truth), `[Static]` lines (every frame of a
         track replaced by the track's best-score box) and <dir of --track>/static/static.pkl: det_annos with the
         detection of every scored track-frame rewritten to that best box and its score (static_init.py:252-284);
dynamic  `[Init]` lines for the dynamic tracks, pedestrians included (dynamic_init.py:125-137);
labels   `mIOU of track` / `mIOU of static`: the best 3D IoU over a frame's GT boxes of the tracker's best box and of
         a refined static label (tools/eval.py:38-101; the labels file is read as that script reads it).

On the host: reading the pickles (each annotation file once, through eval.Annos), np.linalg.inv of the poses and the
flattening into tables (flatten). On the device: transform_box, the size / heading class round trips, the IoU, the
thresholds and the sums — bitwise reproducible, see include/dal3.h — and the det_annos rewrite (post.WritebackPlan,
dal3_writeback_boxes in its static mode with the tracks' best GLOBAL boxes and identity `pose_best`).

Differences from the reference, all deliberate:
  * the IoU of a pair is the rotated-box IoU of iou.py on the float64 boxes the reference hands to its geometry, in
    place of the un-vendored fpointnet_train.provider_fpointnet (compute_box3d_iou) and of pcdet's boxes_iou3d_gpu
    (tools/eval.py): the substitution of eval.box_metrics (see that module's docstring and DESIGN.md);
  * a track type the script asserts on (anything but 1 / 4 for static, 1 / 2 / 4 for dynamic) is scored at 3D IoU >=
    0.5 and counted in one extra line, eval.py's convention for that case;
  * the sums are float64 sums of the float32 per-sample IoUs (NumPy of the reference's time; today's NumPy adds
    `0.0 + np.float32` in float32): the printed .4f digits agree on inputs of the fixtures' size;
  * `static/` is created when missing (the reference fails), and an empty sample set prints nan (ZeroDivisionError).
"""
import argparse
import pathlib
import pickle

import numpy as np
import torch

from . import _hip, eval as ev, iou, post

THR_TYPE = (0.7, 0.5, 0.5)                          # 3D IoU threshold of type 1, 2, 4 (dynamic_init.py:105-114)
THR_OTHER = ev.IOU3D_THRESHOLD_OTHER                # any other type (the reference asserts)
OKBLUE, ENDC = "\033[94m", "\033[0m"                # tools/eval.py:8-14
_INFO = f"[{OKBLUE}Info{ENDC}]"


# ---------------------------------------------------------------------------------------------- device calls
class ScoreAccumulator:
    """dal3_score_acc on the device: score_tracks(..., acc=this) adds a call's sums into it with no host read, so the
    track files of a split accumulate; counts() / result() read it once."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        # 2 float64 sums, then 7 uint64 counts, held as 9 int64 words
        self.acc = torch.zeros(9, dtype=torch.int64, device=self.device)

    def reset(self):
        self.acc.zero_()

    def counts(self):
        """the raw accumulator (one device->host read): float64 sums and integer counts"""
        w = self.acc.cpu()
        f = w[:2].view(torch.float64).tolist()
        n = w[2:].tolist()
        return {"sum_iou_bev": f[0], "sum_iou_3d": f[1], "n_iou_3d_pass": n[0], "n_type1": n[1], "n_type2": n[2],
                "n_type4": n[3], "n_other_type": n[4], "n_scored": n[5], "n_samples": n[6]}

    def result(self):
        """counts() plus iou2d, iou3d, acc as the reference divides them: by n_samples, ALL samples (nan when 0)"""
        c = self.counts()
        n = c["n_samples"]
        div = (lambda x: x / n) if n else (lambda x: float("nan"))
        c.update(iou2d=div(c["sum_iou_bev"]), iou3d=div(c["sum_iou_3d"]), acc=div(float(c["n_iou_3d_pass"])))
        return c


def _table(t, name, dtype, shape, dev):
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    t = t.to(dev).contiguous()
    _hip.require_gpu(t, name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t


def score_tracks(boxes, box_row, frame, pose_inv, gt, has_gt, types, thr=THR_TYPE, thr_other=THR_OTHER, acc=None,
                 return_boxes=False, max_workgroups=0, device="cuda"):
    """dal3_score_tracks on flat tables (tensors on the GPU, or arrays that are uploaded): boxes (R,7) float64 global
    track boxes, box_row (S) / frame (S) int32, pose_inv (F,16) float64, gt (S,7) float32 or float64, has_gt (S) uint8,
    types (S) int32. One launch (two with `acc`, a ScoreAccumulator), no host read.
    Returns (iou_bev (S,), iou_3d (S,)) float32 on the device, NaN where a sample has no ground truth; with
    return_boxes also (pred_box (S,7), label_box (S,7)) float64: the two boxes the reference hands to its geometry."""
    dev = acc.device if acc is not None else (boxes.device if torch.is_tensor(boxes) and boxes.is_cuda else torch.device(device))
    S = int(box_row.shape[0])
    boxes = _table(boxes, "boxes", torch.float64, (boxes.shape[0], 7), dev)
    pose_inv = _table(pose_inv, "pose_inv", torch.float64, (pose_inv.shape[0], 16), dev)
    box_row = _table(box_row, "box_row", torch.int32, (S,), dev)
    frame = _table(frame, "frame", torch.int32, (S,), dev)
    has_gt = _table(has_gt, "has_gt", torch.uint8, (S,), dev)
    types = _table(types, "types", torch.int32, (S,), dev)
    gt = _table(gt, "gt", None, (S, 7), dev)
    if gt.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"gt must be float32 or float64, got {gt.dtype}")
    a = _hip.ScoreArgs()
    a.S, a.R, a.F = S, boxes.shape[0], pose_inv.shape[0]
    a.boxes, a.box_row, a.frame, a.pose_inv = _hip.ptr(boxes), _hip.ptr(box_row), _hip.ptr(frame), _hip.ptr(pose_inv)
    a.gt, a.has_gt, a.type = _hip.ptr(gt), _hip.ptr(has_gt), _hip.ptr(types)
    a.gt_f64 = int(gt.dtype == torch.float64)
    a.max_workgroups = int(max_workgroups)
    a.thr = (_hip.C.c_float * 3)(*[float(x) for x in thr])
    a.thr_other = float(thr_other)
    vb = torch.empty(S, dtype=torch.float32, device=dev)
    v3 = torch.empty(S, dtype=torch.float32, device=dev)
    a.iou_bev, a.iou_3d = _hip.ptr(vb), _hip.ptr(v3)
    out = (vb, v3)
    if return_boxes:
        pb = torch.empty((S, 7), dtype=torch.float64, device=dev)
        lb = torch.empty((S, 7), dtype=torch.float64, device=dev)
        a.pred_box, a.label_box = _hip.ptr(pb), _hip.ptr(lb)
        out = (vb, v3, pb, lb)
    if acc is not None:
        need = _hip.lib().dal3_score_workspace_bytes(S)
        ws = _hip.workspace(need, dev)
        a.acc, a.workspace, a.workspace_bytes = _hip.ptr(acc.acc), _hip.ptr(ws), need
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().dal3_score_tracks(a, _hip.stream()))
    return out


def best_gt_iou(queries, gt_offsets, gt_boxes, query_frame, max_workgroups=0):
    """dal3_best_gt_iou: queries (Q,7) and gt_boxes (G,7) CUDA tensors of one dtype (float32 / float64), gt_offsets
    (F+1) int64, query_frame (Q) int32. Returns (best_iou_3d (Q,), best_iou_bev (Q,)) float32 and best_index (Q,) int32:
    the maximum over the query's own frame's GT boxes of iou.boxes_iou3d (the same bits), the BEV IoU of that pair and
    the first arg-max within the frame; NaN and -1 for a frame without GT boxes."""
    q, g = iou._boxes(queries, "queries"), iou._boxes(gt_boxes, "gt_boxes")
    if q.dtype != g.dtype:
        raise TypeError(f"queries and gt_boxes differ in dtype ({q.dtype} vs {g.dtype})")
    dev, Q = q.device, q.shape[0]
    gt_offsets = _table(gt_offsets, "gt_offsets", torch.int64, (gt_offsets.shape[0],), dev)
    query_frame = _table(query_frame, "query_frame", torch.int32, (Q,), dev)
    if gt_offsets.shape[0] < 1:
        raise ValueError("gt_offsets must hold F + 1 values")
    a = _hip.BestGtArgs()
    a.Q, a.F, a.G = Q, gt_offsets.shape[0] - 1, g.shape[0]
    a.queries, a.query_frame, a.gt_offsets, a.gt_boxes = _hip.ptr(q), _hip.ptr(query_frame), _hip.ptr(gt_offsets), _hip.ptr(g)
    a.boxes_f64 = iou._F64[q.dtype]
    a.max_workgroups = int(max_workgroups)
    v3 = torch.empty(Q, dtype=torch.float32, device=dev)
    vb = torch.empty(Q, dtype=torch.float32, device=dev)
    idx = torch.empty(Q, dtype=torch.int32, device=dev)
    a.best_iou_3d, a.best_iou_bev, a.best_index = _hip.ptr(v3), _hip.ptr(vb), _hip.ptr(idx)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().dal3_best_gt_iou(a, _hip.stream()))
    return v3, vb, idx


# ---------------------------------------------------------------------------------------------- host flattening
def flatten(track, annos):
    """The samples of calculate_init_iou / calculate_static_iou as flat NumPy tables: every (track, frame) of `track` in
    dict order then frame order (static_init.py:65-72). annos: an eval.Annos (each pickle is read once).

    Returns a dict: boxes (S,7) float64 the tracks' global boxes (row s = sample s); own_row = arange(S) and best_row (S)
    int32 = the row of the track's first best-score frame (np.argmax); frame (S) int32 into tokens / pose_inv (F,16)
    float64 = np.linalg.inv(veh_to_global) per distinct frame; gt (S,7) = box[[0,1,2,3,4,5,-1]] of the LAST object
    named match[-1] in the sample's frame, in the annotations' dtype (float32 unless one of them is float64), zeros
    where has_gt (S) uint8 is 0; types (S) int32; track_of (S) / frame_of (S) int64; track_first (T+1) int64; max_score
    (T) the tracks' np.max(score); n_samples = S."""
    tracks = list(track.values())
    lens = np.array([len(v["token"]) for v in tracks], np.int64)
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    S = int(first[-1])
    boxes = np.zeros((S, 7), np.float64)
    types = np.zeros(S, np.int32)
    best_row = np.zeros(S, np.int32)
    frame = np.zeros(S, np.int32)
    has_gt = np.zeros(S, np.uint8)
    max_score = []
    tokens, index, by_name, found = [], {}, [], []
    for i, v in enumerate(tracks):
        lo, hi = int(first[i]), int(first[i + 1])
        score = np.stack(v["score"]) if hi > lo else np.zeros(0, np.float32)
        max_score.append(np.max(score) if hi > lo else np.float32("nan"))
        if hi == lo:
            continue
        boxes[lo:hi] = np.vstack(v["bbox"])
        types[lo:hi] = np.stack(v["type"])
        best_row[lo:hi] = lo + int(np.argmax(score))
        name = v["match"][-1]
        for j, tok in enumerate(v["token"]):
            f = index.get(tok)
            if f is None:
                f = index[tok] = len(tokens)
                tokens.append(tok)
                by_name.append({obj["name"]: obj["box"] for obj in annos(tok)["objects"]})     # the last of a name stays
            frame[lo + j] = f
            g = by_name[f].get(name)
            if g is not None:
                has_gt[lo + j] = 1
                found.append(g)
    idx7 = [0, 1, 2, 3, 4, 5, -1]
    f64 = any(np.asarray(g).dtype == np.float64 for g in found)
    gt = np.zeros((S, 7), np.float64 if f64 else np.float32)
    if found:
        gt[has_gt != 0] = np.stack([np.asarray(g).reshape(-1) for g in found])[:, idx7]
    pose_inv = np.stack([np.linalg.inv(np.reshape(annos(t)["veh_to_global"], [4, 4])).reshape(16) for t in tokens]) \
        if tokens else np.zeros((0, 16))
    return {"boxes": boxes, "own_row": np.arange(S, dtype=np.int32), "best_row": best_row, "frame": frame, "tokens": tokens,
            "pose_inv": pose_inv.astype(np.float64), "gt": gt, "has_gt": has_gt, "types": types,
            "track_of": np.repeat(np.arange(len(tracks)), lens), "frame_of": np.arange(S) - np.repeat(first[:-1], lens),
            "track_first": first, "max_score": max_score, "n_samples": S}


class _Tables:
    """flatten()'s tables on the device, uploaded once for both flavours of a run"""

    def __init__(self, flat, device):
        dev = torch.device(device)
        self.flat = flat
        self.t = {k: torch.from_numpy(np.ascontiguousarray(flat[k])).to(dev)
                  for k in ("boxes", "own_row", "best_row", "frame", "pose_inv", "gt", "has_gt", "types")}
        self.device = dev

    def score(self, best):
        acc = ScoreAccumulator(self.device)
        t = self.t
        score_tracks(t["boxes"], t["best_row" if best else "own_row"], t["frame"], t["pose_inv"], t["gt"], t["has_gt"],
                     t["types"], acc=acc)
        return acc.result()


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _print_lines(tag, r, dynamic):
    """the three lines of calculate_init_iou / calculate_static_iou, character for character"""
    if dynamic:
        print(f"[{tag}] #Vehicle: {r['n_type1']}, #Pedestrian: {r['n_type2']}, #Cyclist: {r['n_type4']}")
        other = r["n_other_type"]
    else:
        print(f"[{tag}] #Vehicle: {r['n_type1']}, #Cyclist: {r['n_type4']}")
        other = r["n_other_type"] + r["n_type2"]
    print(f"[{tag}] Box IoU (2D/3D): {r['iou2d']:.4f}/{r['iou3d']:.4f}")
    print(f"[{tag}] Box estimation accuracy: {r['acc']:.4f}")
    if other:
        print(f"[{tag}] {other} sample(s) of a type other than {'1 / 2 / 4' if dynamic else '1 / 4'} scored at 3D IoU >= "
              f"{THR_OTHER}")


# ---------------------------------------------------------------------------------------------- the three runs
def run_static(track_path, infos_path, det_annos_path, device="cuda"):
    """main() of tools/static_init.py:252-284. Returns {"init": ..., "static": ... (ScoreAccumulator.result() dicts),
    "det_annos": the rewritten list, "result_path"}."""
    track = _load(track_path)
    infos = ev.reorganize_info(_load(infos_path))
    det_annos = ev.sort_detections(_load(det_annos_path))
    annos = ev.Annos(infos)
    token2idx = ev.token_to_det_index(infos, det_annos, annos)
    track = ev.preprocessing(track, annos)
    flat = flatten(track, annos)
    tables = _Tables(flat, device)
    init = tables.score(best=False)
    _print_lines("Init", init, dynamic=False)
    stat = tables.score(best=True)
    # calculate_static_iou:220-229 — the detection next to every scored sample's OWN box gets the track's best box moved
    # into that frame, and the best score; rows and winners come from the write-back kernel's match / owner
    tracks = list(track.values())
    if flat["n_samples"]:
        tokens = sorted(flat["tokens"], key=lambda t: token2idx[t])
        v2g = {t: annos.pose(t) for t in tokens}
        dets = {t: det_annos[token2idx[t]]["boxes_lidar"] for t in tokens}
        has_gt = {(int(i), tracks[i]["token"][int(j)]): bool(h)
                  for i, j, h in zip(flat["track_of"], flat["frame_of"], flat["has_gt"])}
        best_global = flat["boxes"][flat["best_row"][flat["track_first"][:-1]]]
        plan = post.WritebackPlan(tracks, v2g, has_gt, dets, static=True, device=device,
                                  pose_best=np.tile(np.eye(4).reshape(16), (len(tracks), 1)))
        new, _ = plan.apply(best_global)                    # AssertionError('Bounding box not in det_annos.') as there
        owner = plan.owner.cpu().numpy()
        for t in tokens:
            d = det_annos[token2idx[t]]
            d["boxes_lidar"][...] = new[t].astype(d["boxes_lidar"].dtype, copy=False)
            own = owner[plan.start[t]:plan.start[t] + plan.lens[t]]
            for k in np.nonzero(own >= 0)[0]:
                d["score"][k] = flat["max_score"][plan.track_of_pair[own[k]]]
    result_dir = pathlib.Path(track_path).parent / "static"
    result_dir.mkdir(parents=True, exist_ok=True)
    result_path = result_dir / "static.pkl"
    with open(result_path, "wb") as f:
        pickle.dump(det_annos, f)
    _print_lines("Static", stat, dynamic=False)
    return {"init": init, "static": stat, "det_annos": det_annos, "result_path": result_path}


def run_dynamic(track_path, infos_path, device="cuda"):
    """main() of tools/dynamic_init.py:125-137. Returns {"init": ScoreAccumulator.result()}."""
    track = _load(track_path)
    annos = ev.Annos(ev.reorganize_info(_load(infos_path)))
    init = _Tables(flatten(track, annos), device).score(best=False)
    _print_lines("Init", init, dynamic=True)
    return {"init": init}


def run_labels(track_path, infos_path, static_path, device="cuda"):
    """main() of tools/eval.py:38-101. Returns {"iou_track", "iou_static" (float32 arrays), "miou_track",
    "miou_static"}."""
    print(f"{_INFO} Load track data")
    track = _load(track_path)
    print(f"{_INFO} Load infos data")
    annos = ev.Annos(ev.reorganize_info(_load(infos_path)))
    print(f"{_INFO} Load static data")
    static = _load(static_path)
    index, offsets, gts, frame, best, label = {}, [0], [], [], [], []
    for ID, obj in static.items():
        tok = obj["token"]
        if tok not in index:
            index[tok] = len(index)
            boxes = np.array([o["box"] for o in annos(tok)["objects"]])
            if boxes.ndim != 2 or not len(boxes):
                raise ValueError(f"frame {tok!r} of label {ID!r} has no ground-truth object")      # an IndexError there
            gts.append(boxes[:, [0, 1, 2, 3, 4, 5, -1]].astype(np.float32))
            offsets.append(offsets[-1] + len(boxes))
        frame.append(index[tok])
        best.append(np.asarray(track[ID]["bbox"][int(np.argmax(track[ID]["score"]))], np.float64).reshape(7))
        label.append(np.asarray(obj["bbox"], np.float32).reshape(7))
    Q = len(frame)
    if Q:
        tokens = list(index)
        inv = np.stack([np.linalg.inv(np.reshape(annos(t)["veh_to_global"], [4, 4])) for t in tokens])
        query = np.concatenate([ev._transform(np.stack(best), inv[np.asarray(frame)]).astype(np.float32), np.stack(label)])
        dev = torch.device(device)
        v3, _, _ = best_gt_iou(torch.from_numpy(query).to(dev), torch.tensor(offsets, dtype=torch.int64),
                               torch.from_numpy(np.concatenate(gts)).to(dev), torch.tensor(frame + frame, dtype=torch.int32))
        v3 = v3.cpu().numpy()
        iou_track, iou_static = v3[:Q], v3[Q:]
        iou_static = iou_static[~(iou_static > 1)]          # `if static_iou > 1: continue`, the static list only
    else:
        iou_track = iou_static = np.zeros(0, np.float32)
    mean = lambda x: np.mean(x) if len(x) else np.float32("nan")   # noqa: E731
    out = {"iou_track": iou_track, "iou_static": iou_static, "miou_track": mean(iou_track), "miou_static": mean(iou_static)}
    print(f"{_INFO} mIOU of track: {out['miou_track']}")
    print(f"{_INFO} mIOU of static: {out['miou_static']}")
    return out


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = parser.add_subparsers(dest="run", required=True)
    p = sub.add_parser("static", help="[Init] / [Static] lines and static/static.pkl (tools/static_init.py)")
    p.add_argument("--track", required=True, help="Path to trackStatic.pkl.")
    p.add_argument("--infos", required=True, help="Path to infos file.")
    p.add_argument("--det_annos", required=True, help="Path to detection annos.")
    p = sub.add_parser("dynamic", help="[Init] lines of the dynamic tracks (tools/dynamic_init.py)")
    p.add_argument("--track", required=True, help="Path to trackDynamic.pkl.")
    p.add_argument("--infos", required=True, help="Path to infos file.")
    p = sub.add_parser("labels", help="mIOU of the tracker's best boxes and of refined static labels (tools/eval.py)")
    p.add_argument("--track", required=True, help="Path to track.pkl.")
    p.add_argument("--infos", required=True, help="Path to infos file.")
    p.add_argument("--static", required=True, help="Path to static_labels.pkl.")
    args = parser.parse_args(argv)
    if args.run == "static":
        run_static(args.track, args.infos, args.det_annos)
    elif args.run == "dynamic":
        run_dynamic(args.track, args.infos)
    else:
        run_labels(args.track, args.infos, args.static)


if __name__ == "__main__":
    main()
