"""File-level drivers of the auto-labeling run: `tools/static_eval.py` and `tools/dynamic_eval.py` of the reference
with every per-item Python step replaced by the batched device path of this package —

    trackStatic.pkl / trackDynamic.pkl + infos + annos/*.pkl + det_annos.pkl        (SURVEY.md 8(g) formats)
      -> crop preparation on the device            prep.prepare_*_batch            (N1; *TRACK.__getitem__)
      -> the heads + box decode                    model.refine                    (8(a); test_one_epoch)
      -> one all-gather of the boxes over RCCL when launched on several GPUs       (8(e))
      -> write-back into det_annos on the device   post.writeback_*                (N3; postprocessing)
      -> static/box/{model_type}.pkl / dynamic/box/box.pkl

Same command line as the reference's scripts (static_eval.py:291-299, dynamic_eval.py:247-254):

    python -m 3dal_pytorch_amd.eval static  --track trackStatic.pkl  --infos infos.pkl --model_path x.pth \
                                            --model_type one_box_est --det_annos det_annos.pkl
    python -m 3dal_pytorch_amd.eval dynamic --track trackDynamic.pkl --infos infos.pkl --model_path x.pth \
                                            --det_annos det_annos.pkl

Differences from the reference, all deliberate:
  * every annotation pickle is read once per run (the reference re-reads one per item, per frame and per
    window slot: static_model.py:536, static_eval.py:78,85, dynamic_model.py:449,464);
  * `--sampler numpy` (default) consumes the global NumPy stream in the reference's order — per batch the
    items' resampling draws, then the crops' object-point draws — so the same seed gives the same crops;
    `--sampler device` draws on the GPU from a counter-based generator keyed on the global item index, which is
    what a multi-GPU launch needs (a sharded run cannot share one host stream) and what throughput runs use;
  * a dynamic item whose own frame lacks the matched annotation: the reference's Dataset returns a RANDOM other
    item in its place (dynamic_model.py:487-489) and `postprocessing` then skips that frame
    (dynamic_eval.py:88-89), i.e. the substitute's box is computed and never read. With the numpy sampler this
    is reproduced draw for draw (the item's window draws, `randint`, the substitute's, recursively) so that every
    later item sees the reference's stream; with the device sampler the item itself is refined — either way the
    row is one the write-back does not use;
  * the two `[Eval]` lines `postprocessing` logs (Box IoU 2D/3D, box estimation accuracy) come from box_metrics():
    the same samples, boxes, thresholds and denominators as the reference's metric loop, with one substitution. The
    reference scores each pair with compute_box3d_iou (tools/utils.py:81-103), whose geometry lives in the
    un-vendored fpointnet_train.provider_fpointnet; here it is the rotated-box IoU of iou.py (BEV overlap of the
    [x, y, z, l, w, h, yaw] rectangles, 3D = BEV overlap x z overlap over the union of the volumes, the formula of
    the reference's det3d/ops/iou3d_nms). The printed numbers therefore follow the same recipe but are not the
    reference's digits wherever that helper's geometry differs. Two more departures: a track type other than 1 / 4
    (an assertion there) uses the 0.5 threshold and is counted in one extra log line, and an empty sample set (a
    ZeroDivisionError there) logs nan. The product of the run — the rewritten det_annos — is unchanged by them.
"""
import argparse
import logging
import os
import pathlib
import pickle
import random

import numpy as np
import torch
import torch.distributed as dist

from . import dist as sharding
from . import arch, post, prep

SEED = 10922081                                     # static_eval.py:303
IOU3D_THRESHOLD = {1: 0.7, 4: 0.5}                  # box estimation accuracy by track type (static_eval.py:136-140)
IOU3D_THRESHOLD_OTHER = 0.5                         # any other type (the reference asserts)


def fix_seed(seed=SEED):
    """tools/utils.py:24-29"""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def reorganize_info(infos):
    """list of info dicts -> {token: info} (tools/utils.py:46-51)"""
    return {info["token"]: info for info in infos}


def sort_detections(detections):
    """det_annos ordered by frame_id (static_eval.py:169-176)"""
    rank = np.argsort(np.array([det["frame_id"] for det in detections]))
    return [detections[r] for r in rank]


class Annos:
    """The per-frame annotation pickles ({split}/annos/*.pkl), each read at most once."""

    def __init__(self, infos):
        self.infos = infos
        self._cache = {}

    def __call__(self, token):
        a = self._cache.get(token)
        if a is None:
            with open(self.infos[token]["anno_path"], "rb") as f:
                a = pickle.load(f)
            self._cache[token] = a
        return a

    def pose(self, token):
        """flat-16 veh_to_global of the frame"""
        return np.asarray(self(token)["veh_to_global"], np.float64).reshape(16)

    def gt_box(self, token, name):
        """the (9,) `box` of the annotation called `name` in that frame, or None (the last object of that
        name, as the reference's loops without `break` leave it: static_eval.py:106-108; names are unique per frame)."""
        box = None
        for obj in self(token)["objects"]:
            if obj["name"] == name:
                box = obj["box"]
        return box


def token_to_det_index(infos, det_annos, annos):
    """{token: row of det_annos} through 'segment-{scene}_with_camera_labels_{frame:03d}' (static_eval.py:368-376)"""
    by_frame = {d["frame_id"]: i for i, d in enumerate(det_annos)}
    out = {}
    for token in infos:
        a = annos(token)
        out[token] = by_frame[f"segment-{a['scene_name']}_with_camera_labels_{a['frame_id']:03d}"]
    return out


def preprocessing(track, annos):
    """drop the static tracks whose best-score frame lacks the matched annotation (static_eval.py:26-44)"""
    for k in [k for k, v in track.items()
              if annos.gt_box(v["token"][int(np.argmax(np.stack(v["score"])))], v["match"][-1]) is None]:
        del track[k]
    return track


def _world(group):
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def _check_sampler(sampler, group):
    if sampler not in ("numpy", "device"):
        raise ValueError(f"unknown sampler {sampler!r}")
    if sampler == "numpy" and _world(group)[1] > 1:
        raise ValueError("sampler='numpy' draws from one host stream and cannot be sharded; use sampler='device'")


def refine_static_tracks(model, track, annos, batch_size=64, n_points=4096, sampler="numpy", seed=SEED, group=None):
    """`test_one_epoch` of static_eval.py:255-289 over STATICTRACK(track): (n_tracks, 7) float64 refined boxes,
    one per track, in the vehicle frame of the track's best-score frame. On several ranks each refines a
    contiguous range of tracks and the boxes are all-gathered once."""
    _check_sampler(sampler, group)
    tracks = list(track.values())
    n = len(tracks)
    dev = next(model.parameters()).device
    model.eval()
    model.sampler, model.seed = sampler, seed
    rank, world = _world(group)
    lo, hi = sharding.shard_range(n, rank, world)
    local = torch.zeros((hi - lo, 7), dtype=torch.float32, device=dev)
    for a in range(lo, hi, batch_size):
        b = min(a + batch_size, hi)
        chunk = tracks[a:b]
        poses = [annos.pose(t["token"][int(np.argmax(np.stack(t["score"])))]) for t in chunk]
        pts, init = prep.prepare_static_batch(chunk, poses, n_points=n_points, sampler=sampler, seed=seed,
                                              item_offset=a, device=dev)
        model.item_offset = a
        local[a - lo:b - lo] = model.refine(pts, init)
    model.item_offset = 0
    return sharding.all_gather_boxes(local, n, group).double().cpu().numpy()


def _dynamic_items(track, annos):
    """[(track_index, frame_index, has_gt)] in DYNAMICTRACK's index order (dynamic_model.py:406-424)"""
    items = []
    for t, v in enumerate(track.values()):
        for i, tok in enumerate(v["token"]):
            items.append((t, i, annos.gt_box(tok, v["match"][-1]) is not None))
    return items


def numpy_stream_parts(batch, items, tracks, r, n_per_frame, prepare):
    """The dynamic Dataset's substitution on the global NumPy stream, for one batch of dataset indices: an item whose
    own frame lacks the matched annotation makes its window draws, then `np.random.randint(len(items))` picks the
    item that takes its place (dynamic_model.py:487-489), recursively. prepare(list of indices) runs on every run of
    items that can be prepared, in stream order; returns the list of its results."""
    n = len(items)
    parts, seg = [], []
    for k in batch:
        k = int(k)
        while not items[k][2]:                              # replaced item: its draws, then the pick of its substitute
            if seg:
                parts.append(prepare(seg))
                seg = []
            t, it, _ = items[k]
            for i in range(it - r, it + r + 1):
                if 0 <= i < len(tracks[t]["point"]) and len(tracks[t]["point"][i]) > 0:
                    np.random.choice(len(tracks[t]["point"][i]), n_per_frame, replace=True)
            k = int(np.random.randint(n))
        seg.append(k)
    parts.append(prepare(seg))
    return parts


def join_dynamic_parts(parts):
    """prepare_dynamic_batch results of consecutive runs -> one batch; pts and box joined in the point-major storage
    their views come from, a label dict (4th value, if any) joined per key"""
    if len(parts) == 1:
        return parts[0]
    out = [torch.cat([p[0].transpose(2, 1) for p in parts], 0).transpose(2, 1),
           torch.cat([p[1].transpose(2, 1) for p in parts], 0).transpose(2, 1),
           torch.cat([p[2] for p in parts], 0)]
    if len(parts[0]) > 3:
        out.append({key: torch.cat([p[3][key] for p in parts], 0) for key in parts[0][3]})
    return tuple(out)


def refine_dynamic_tracks(model, track, annos, batch_size=64, n_per_frame=1024, sampler="numpy", seed=SEED, group=None):
    """`test_one_epoch` of dynamic_eval.py:213-245 over DYNAMICTRACK(track): (sum of track lengths, 7) float64,
    one refined box per track-frame in that frame's vehicle frame (see the module docstring for the rows of
    frames without the matched annotation, which the write-back never reads)."""
    _check_sampler(sampler, group)
    tracks = list(track.values())
    items = _dynamic_items(track, annos)
    n = len(items)
    dev = next(model.parameters()).device
    model.eval()
    model.sampler, model.seed = sampler, seed
    rank, world = _world(group)
    lo, hi = sharding.shard_range(n, rank, world)
    local = torch.zeros((hi - lo, 7), dtype=torch.float32, device=dev)

    store = prep.TrackStore(tracks, dev)                    # every frame of every track, uploaded once

    def prepare(idx, first):
        """(pts, box, init) of items[idx]; the device generator is keyed on first + row"""
        return prep.prepare_dynamic_batch(store, [items[k][:2] for k in idx],
                                          [annos.pose(tracks[items[k][0]]["token"][items[k][1]]) for k in idx],
                                          n_per_frame=n_per_frame, r=model.r, s=model.s, sampler=sampler, seed=seed,
                                          item_offset=first, device=dev)

    for a in range(lo, hi, batch_size):
        b = min(a + batch_size, hi)
        if sampler == "device":
            pts, box, init = prepare(list(range(a, b)), a)
        else:
            parts = numpy_stream_parts(range(a, b), items, tracks, model.r, n_per_frame, lambda seg: prepare(seg, 0))
            pts, box, init = join_dynamic_parts(parts)[:3]
        model.item_offset = a
        local[a - lo:b - lo] = model.refine(pts, box, init)
    model.item_offset = 0
    return sharding.all_gather_boxes(local, n, group).double().cpu().numpy()


def write_back(track, annos, token2idx, final_bboxes, det_annos, static):
    """the det_annos rewrite of `postprocessing` (static_eval.py:62-167, dynamic_eval.py:43-141): for every track
    frame that has the matched annotation, the first detection of that frame within 0.1 m of the track's box gets
    the refined box. det_annos is modified in place (like the reference) and returned."""
    tracks = list(track.values())
    tokens = sorted({t for v in tracks for t in v["token"]}, key=lambda t: token2idx[t])
    v2g = {t: annos.pose(t) for t in tokens}
    dets = {t: det_annos[token2idx[t]]["boxes_lidar"] for t in tokens}
    has_gt = {(i, t): annos.gt_box(t, v["match"][-1]) is not None for i, v in enumerate(tracks) for t in v["token"]}
    fn = post.writeback_static if static else post.writeback_dynamic
    new, _ = fn(tracks, v2g, has_gt, final_bboxes, dets)
    for t in tokens:
        rows = det_annos[token2idx[t]]["boxes_lidar"]
        rows[...] = new[t].astype(rows.dtype, copy=False)
    return det_annos


def _angle_class_round_trip(angle):
    """class2angle(*angle2class(angle, 12)) of tools/utils.py:53-77, elementwise on an array with the same operations
    in the same order and precision as the reference's scalar code: angle2class runs in the angle's own dtype (a
    float32 annotation heading stays float32 there, the Python floats it meets are cast to it), class2angle in float64"""
    angle = np.asarray(angle)
    dt = angle.dtype.type
    per = 2 * np.pi / float(arch.NUM_HEADING_BIN)
    angle = np.mod(angle, dt(2 * np.pi))
    shifted = np.mod(angle + dt(per / 2), dt(2 * np.pi))
    cls = (shifted / dt(per)).astype(np.int64)
    residual = shifted - (cls * per + per / 2).astype(angle.dtype)
    out = cls * per + residual.astype(np.float64)
    return np.where(out > np.pi, out - 2 * np.pi, out)


def _size_class_round_trip(lwh):
    """class2size(*size2class(lwh)) of tools/utils.py:62-81, rowwise on (S, 3) float64"""
    mean = np.array(arch.MEAN_SIZE, np.float64)
    cls = np.argmin(np.linalg.norm(lwh[:, None, :] - mean[None], axis=2), axis=1)
    return mean[cls] + (lwh - mean[cls])


def _transform(box, pose):
    """transform_box of static_eval.py:46-60 on (S, 7) boxes with (S, 4, 4) poses"""
    heading = box[:, 6] + np.arctan2(pose[:, 1, 0], pose[:, 0, 0])
    center = np.einsum("sij,sj->si", pose[:, :3, :3], box[:, :3]) + pose[:, :3, 3]
    return np.concatenate([center, box[:, 3:6], heading[:, None]], axis=1)


def metric_samples(track, annos, final_bboxes, static):
    """The samples of `postprocessing`'s metric loop (static_eval.py:62-141, dynamic_eval.py:43-119) and the boxes it
    hands to compute_box3d_iou, built on the host in float64 without a per-sample loop over the arithmetic.

    static: one sample per (track, frame) whose frame has the matched annotation; the refined box goes to the global
    frame through the best-score frame's pose and into the sample frame's vehicle frame. Its heading, and the ground
    truth's, are taken RELATIVE to the track's best box in that frame (`init_box`) and sent through
    angle2class -> class2angle; centres are not rotated (the reference's quirk, kept). n_samples counts EVERY frame of
    the tracks, with or without ground truth (static_eval.py:83).
    dynamic: one sample per track-frame with ground truth; headings absolute; n_samples = the number of samples.
    Sizes of both boxes go through size2class -> class2size.

    Returns {"pred": (S,7), "gt": (S,7) float64 [x,y,z,l,w,h,yaw], "types": (S,) int64, "track": (S,), "frame": (S,)
    int64 indices, "n_samples": int}."""
    tracks = list(track.values())
    final = np.asarray(final_bboxes, np.float64).reshape(-1, 7)
    t_idx, f_idx, rows, gts = [], [], [], []
    index = 0
    for i, v in enumerate(tracks):
        for j, tok in enumerate(v["token"]):
            g = annos.gt_box(tok, v["match"][-1])
            if g is not None:
                t_idx.append(i)
                f_idx.append(j)
                rows.append(i if static else index + j)
                gts.append(np.asarray(g).reshape(-1)[[0, 1, 2, 3, 4, 5, -1]])
        index += len(v["token"])
    S = len(rows)
    n_samples = index if static else S
    t_idx, f_idx = np.asarray(t_idx, np.int64), np.asarray(f_idx, np.int64)
    gt_yaw = np.stack(gts)[:, 6] if S else np.zeros(0)     # in the annotation's dtype (see _angle_class_round_trip)
    gt = np.stack(gts).astype(np.float64) if S else np.zeros((0, 7))
    types = np.asarray([tracks[i]["type"][j] for i, j in zip(t_idx, f_idx)], np.int64)
    pred = final[np.asarray(rows, np.int64)] if S else np.zeros((0, 7))
    if static and S:
        best = [v["token"][int(np.argmax(np.stack(v["score"])))] for v in tracks]
        pose_best = np.stack([annos.pose(best[i]).reshape(4, 4) for i in t_idx])
        pose_inv = np.linalg.inv(np.stack([annos.pose(tracks[i]["token"][j]).reshape(4, 4) for i, j in zip(t_idx, f_idx)]))
        best_box = np.stack([np.asarray(tracks[i]["bbox"][int(np.argmax(np.stack(tracks[i]["score"])))], np.float64)
                             .reshape(7) for i in t_idx])
        pred = _transform(_transform(pred, pose_best), pose_inv)
        init = _transform(best_box, pose_inv)
        pred_yaw = _angle_class_round_trip(pred[:, 6] - init[:, 6])
        gt_yaw = _angle_class_round_trip(gt_yaw - init[:, 6])
    else:
        pred_yaw = _angle_class_round_trip(pred[:, 6])
        gt_yaw = _angle_class_round_trip(gt_yaw)
    pred = np.concatenate([pred[:, :3], _size_class_round_trip(pred[:, 3:6]), pred_yaw[:, None]], axis=1)
    gt = np.concatenate([gt[:, :3], _size_class_round_trip(gt[:, 3:6]), gt_yaw[:, None]], axis=1)
    return {"pred": pred, "gt": gt, "types": types, "track": t_idx, "frame": f_idx, "n_samples": int(n_samples)}


def box_metrics(track, annos, final_bboxes, static, device="cuda"):
    """The numbers `postprocessing` logs: mean BEV IoU, mean 3D IoU and the box estimation accuracy (3D IoU >= 0.7
    for type 1, >= 0.5 for type 4 and, here, for any other type), each summed over metric_samples()'s samples and
    divided by its n_samples (nan when that is 0). One paired_iou launch on `device`.

    Returns metric_samples()'s dict plus "iou2d", "iou3d", "acc" (floats), "iou_bev", "iou_3d" (S,) float32 per
    sample, "n_correct" and "n_other_type" (ints)."""
    from . import iou
    out = metric_samples(track, annos, final_bboxes, static)
    S = out["pred"].shape[0]
    dev = torch.device(device)
    if S:
        vb, v3 = iou.paired_iou(torch.from_numpy(out["pred"]).to(dev), torch.from_numpy(out["gt"]).to(dev))
        vb, v3 = vb.cpu().numpy(), v3.cpu().numpy()
    else:
        vb, v3 = np.zeros(0, np.float32), np.zeros(0, np.float32)
    types = out["types"]
    thr = np.full(S, IOU3D_THRESHOLD_OTHER)
    for t, th in IOU3D_THRESHOLD.items():
        thr[types == t] = th
    n_correct = int(np.sum(v3 >= thr))
    n = out["n_samples"]
    mean = (lambda x: float(x) / n) if n else (lambda x: float("nan"))
    out.update(iou_bev=vb, iou_3d=v3, iou2d=mean(np.sum(vb, dtype=np.float64)), iou3d=mean(np.sum(v3, dtype=np.float64)),
               acc=mean(n_correct), n_correct=n_correct, n_other_type=int(np.sum(~np.isin(types, list(IOU3D_THRESHOLD)))))
    return out


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _logger(log_file):
    """console + file, as tools/utils.py:31-44; the handlers belong to one run() and are closed by it"""
    logger = logging.getLogger("3dal_pytorch_amd.eval")
    logger.setLevel(logging.INFO)
    logger.propagate = False
    fmt = logging.Formatter("%(asctime)s  %(levelname)5s  %(message)s")
    for h in (logging.StreamHandler(), logging.FileHandler(filename=log_file, mode="w")):
        h.setFormatter(fmt)
        logger.addHandler(h)
    return logger


def run(head, track_path, infos_path, det_annos_path, model_path, model_type="one_box_est", batch_size=64,
        sampler="numpy", device="cuda", result_path=None, group=None, precision="fp32"):
    """`main()` of static_eval.py:291-397 (head='static') / dynamic_eval.py:247-309 (head='dynamic').
    Returns (final_bboxes, det_annos); rank 0 writes the result pickle where the reference writes it."""
    from . import dynamic_model, static_model
    fix_seed(SEED)
    root = pathlib.Path(track_path).parent / head
    rank, _ = _world(group)
    result_path = pathlib.Path(result_path) if result_path else \
        root / "box" / (f"{model_type}.pkl" if head == "static" else "box.pkl")
    log_dir = root / "log" / "eval"
    if rank == 0:
        result_path.parent.mkdir(parents=True, exist_ok=True)
        log_dir.mkdir(parents=True, exist_ok=True)
    logger = _logger(log_dir / (f"{model_type}.txt" if head == "static" else "eval.txt")) if rank == 0 else None

    def say(msg):
        if logger:
            logger.info(msg)
    try:
        say("Load track data")
        track = _load(track_path)
        say("Load info data")
        infos = reorganize_info(_load(infos_path))
        det_annos = sort_detections(_load(det_annos_path))
        annos = Annos(infos)
        token2idx = token_to_det_index(infos, det_annos, annos)
        if head == "static":
            ctor = {"one_box_est": static_model.StaticModelOneBoxEst, "two_box_est": static_model.StaticModelTwoBoxEst}
            if model_type not in ctor:
                raise ValueError(f'No model supports for model type "{model_type}".')
            track = preprocessing(track, annos)
            model = ctor[model_type](n_classes=3, n_channel=3)
        elif head == "dynamic":
            model = dynamic_model.DynamicModel(n_classes=3, n_channel=4)
        else:
            raise ValueError(f"unknown head {head!r}")
        say(f"Load model from {model_path}")
        model.load_state_dict(torch.load(model_path, map_location="cpu")["model_state_dict"])
        model = model.to(device)
        model.precision = precision                 # "bf16"/"fp16": 16-bit MFMA operands, fp32 accumulate (C3/C5)
        say("Start testing")
        refine = refine_static_tracks if head == "static" else refine_dynamic_tracks
        final_bboxes = refine(model, track, annos, batch_size=batch_size, sampler=sampler, group=group)
        say("Start post processing")
        det_annos = write_back(track, annos, token2idx, final_bboxes, det_annos, static=(head == "static"))
        if rank == 0:
            say(f"Saving results to {result_path}")
            with open(result_path, "wb") as f:
                pickle.dump(det_annos, f)
            m = box_metrics(track, annos, final_bboxes, static=(head == "static"), device=device)
            say(f"[Eval] Box IoU (2D/3D): {m['iou2d']:.4f}/{m['iou3d']:.4f}")
            say(f"[Eval] Box estimation accuracy: {m['acc']:.4f}")
            if m["n_other_type"]:
                say(f"[Eval] {m['n_other_type']} sample(s) of a type other than 1 / 4 scored at 3D IoU >= "
                    f"{IOU3D_THRESHOLD_OTHER}")
        return final_bboxes, det_annos
    finally:
        if logger:
            for h in list(logger.handlers):
                logger.removeHandler(h)
                h.close()


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("head", choices=["static", "dynamic"])
    parser.add_argument("--track", required=True, help="Path to trackStatic.pkl / trackDynamic.pkl.")
    parser.add_argument("--infos", required=True, help="Path to infos file.")
    parser.add_argument("--model_path", required=True, help="Path to model.")
    parser.add_argument("--model_type", default="one_box_est", help="Type of model (static head).")
    parser.add_argument("--det_annos", required=True, help="Path to detection annos.")
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("--sampler", choices=["numpy", "device"], default="numpy")
    parser.add_argument("--precision", choices=["fp32", "f16x3", "bf16", "fp16"], default="fp32",
                        help="MFMA operand type of the shared MLPs (fp32 = the reference's arithmetic).")
    parser.add_argument("--result", default=None, help="Output pickle (default: the reference's location).")
    args = parser.parse_args(argv)
    group = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:                      # launched by torch.distributed.run
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl")
    try:
        run(args.head, args.track, args.infos, args.det_annos, args.model_path, args.model_type, args.batch_size,
            args.sampler, result_path=args.result, group=group, precision=args.precision)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
