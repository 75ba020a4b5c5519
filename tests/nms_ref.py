"""NumPy restatement of dal3_nms / dal3_center_decode (include/dal3.h): test infrastructure, and the seeded inputs of
tests/golden/nms.npz (tests/golden/gen_nms.py runs the reference on them; the tests rebuild them here).

    order(scores)                 the stable order: score descending, NaN first, equal scores by ascending row
    nms(...)                      candidates, greedy scan (rotate: tests/iou_ref.py's float64 IoU, on the boxes converted
                                  as rotate_nms_pcdet converts them with mirror=True; circle: float32), cuts
    decode(...)                   CenterHead.predict's arithmetic and post_processing's masks, float32 step by step
    clustered_scene / head_maps   the inputs
"""
import numpy as np

import iou_ref

# the reference's test configuration (configs/waymo/voxelnet/*.py test_cfg) and a second set where both cuts and every
# face of the range bite; circle_* use circular NMS with a radius per task
CONFIGS = {
    "ref": dict(score_threshold=0.1, post_center_limit_range=[-80.0, -80.0, -10.0, 80.0, 80.0, 10.0], out_size_factor=8,
                voxel_size=[0.1, 0.1], pc_range=[-75.2, -75.2], nms_iou_threshold=0.7, nms_pre_max_size=4096,
                nms_post_max_size=500, circular_nms=False, min_radius=[]),
    "small": dict(score_threshold=0.1, post_center_limit_range=[-74.0, -74.5, -5.0, -64.0, -63.5, 5.0], out_size_factor=8,
                  voxel_size=[0.1, 0.1], pc_range=[-75.2, -75.2], nms_iou_threshold=0.3, nms_pre_max_size=40,
                  nms_post_max_size=10, circular_nms=False, min_radius=[]),
    "circle": dict(score_threshold=0.1, post_center_limit_range=[-80.0, -80.0, -10.0, 80.0, 80.0, 10.0], out_size_factor=8,
                   voxel_size=[0.1, 0.1], pc_range=[-75.2, -75.2], nms_iou_threshold=0.7, nms_pre_max_size=4096,
                   nms_post_max_size=20, circular_nms=True, min_radius=[1.5, 0.6]),
}
HEAD = dict(B=2, H=16, W=16, num_classes=[1, 2])
# the NMS cases of the clustered scene: (mode, thresh, pre_max, post_max)
SCENE_CASES = {"rotate_ref": ("rotate", 0.7, 4096, 500), "rotate_cut": ("rotate", 0.7, 120, 30),
               "circle_ref": ("circle", 1.0, 0, 83), "circle_cut": ("circle", 0.25, 0, 25)}


def as_test_cfg(cfg):
    """a CONFIGS entry as the nested test_cfg CenterHead.predict reads"""
    top = {k: v for k, v in cfg.items() if not k.startswith("nms_")}
    top["nms"] = {k: v for k, v in cfg.items() if k.startswith("nms_")}
    return top


TOKENS = ["seq_0_frame_0.pkl", "seq_0_frame_1.pkl"]


def order(scores):
    s = np.asarray(scores, np.float32)
    nan = np.isnan(s)
    return np.lexsort((np.arange(s.size), np.where(nan, 0.0, -s.astype(np.float64)), ~nan)).astype(np.int64)


def mirrored(boxes):
    """rotate_nms_pcdet's conversion (box_torch_ops.py:255-257) in the boxes' own precision"""
    b = np.array(boxes)[:, [0, 1, 2, 4, 3, 5, -1]]
    b[:, -1] = -b[:, -1] - b.dtype.type(np.pi / 2)
    return b


def suppression(boxes, mode, thresh):
    """(m, m) bool: [i, j] = i suppresses j"""
    if mode == "circle":
        b = np.asarray(boxes)
        dx = (b[:, None, 0] - b[None, :, 0]).astype(np.float32)
        dy = (b[:, None, 1] - b[None, :, 1]).astype(np.float32)
        xx, yy = dx * dx, dy * dy
        with np.errstate(invalid="ignore"):
            return (xx + yy) <= np.float32(thresh)
    iou = iou_ref.pairwise(boxes, boxes)[0]
    with np.errstate(invalid="ignore"):
        return iou > np.float64(np.float32(thresh))


def greedy(sup, limit=0):
    """kept positions of a greedy scan over an (m, m) suppression matrix, stopped at `limit` keeps (0: none)"""
    m = sup.shape[0]
    removed = np.zeros(m, bool)
    kept = []
    for i in range(m):
        if limit and len(kept) >= limit:
            break
        if removed[i]:
            continue
        kept.append(i)
        removed[i + 1:] |= sup[i, i + 1:]
    return np.asarray(kept, np.int64)


def nms(boxes, scores, mode, thresh, pre_max=0, post_max=0, mirror=False):
    """-> the kept rows, best first"""
    o = order(scores)
    if pre_max:
        o = o[:pre_max]
    b = np.asarray(boxes)[o][:, [0, 1, 2, 3, 4, 5, -1]]
    if mirror:
        b = mirrored(b)
    return o[greedy(suppression(b, mode, thresh), post_max)]


def clustered_scene(seed, n_objects=40, max_copies=8):
    """n_objects boxes, each with 1..max_copies jittered copies -> boxes (n, 7) float32, scores (n) float32, all distinct"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_objects):
        c = np.concatenate([rng.uniform(-40, 40, 2), rng.uniform(-1, 1, 1), rng.uniform([3.5, 1.6, 1.4], [5.5, 2.3, 2.0]),
                            rng.uniform(-np.pi, np.pi, 1)])
        for _ in range(int(rng.integers(1, max_copies + 1))):
            j = c.copy()
            j[:2] += rng.normal(0, 0.35, 2)
            j[3:6] *= rng.uniform(0.9, 1.1, 3)
            j[6] += rng.normal(0, 0.1)
            rows.append(j)
    boxes = np.asarray(rows, np.float32)
    scores = rng.permutation(np.linspace(0.12, 0.98, boxes.shape[0])).astype(np.float32)
    return boxes, scores


def head_maps(seed, vel=True, B=HEAD["B"], H=HEAD["H"], W=HEAD["W"], num_classes=HEAD["num_classes"]):
    """per task the network's NCHW float32 outputs: about a third of the cells above the score threshold, boxes a few
    cells long (neighbours overlap), heights beyond the range's z faces now and then"""
    rng = np.random.default_rng(seed)
    out = []
    for C in num_classes:
        d = {"hm": rng.normal(-2.8, 1.4, (B, C, H, W)), "reg": rng.uniform(0, 1, (B, 2, H, W)),
             "height": rng.normal(0, 5.0, (B, 1, H, W)),
             "dim": np.log(np.array([4.0, 1.9, 1.6]))[None, :, None, None] + rng.normal(0, 0.25, (B, 3, H, W)),
             "rot": rng.normal(0, 1, (B, 2, H, W))}
        if vel:
            d["vel"] = rng.normal(0, 3, (B, 2, H, W))
        out.append({k: v.astype(np.float32) for k, v in d.items()})
    return out


def decode(task, cfg):
    """one task's NCHW maps -> per sample (cell (n), label (n), boxes (n, 9 or 7) float32, score (n) float32), the
    survivors in cell order"""
    f = np.float32
    hm = np.transpose(task["hm"], (0, 2, 3, 1))
    B, H, W, _ = hm.shape
    with np.errstate(over="ignore"):
        sig = (f(1) / (f(1) + np.exp(-hm))).astype(f)
    score, label = sig.max(-1), sig.argmax(-1)
    at = lambda k: np.transpose(task[k], (0, 2, 3, 1)).astype(f)   # noqa: E731
    ys, xs = np.meshgrid(np.arange(H, dtype=f), np.arange(W, dtype=f), indexing="ij")
    x = ((xs[None] + at("reg")[..., 0]) * f(cfg["out_size_factor"])) * f(cfg["voxel_size"][0]) + f(cfg["pc_range"][0])
    y = ((ys[None] + at("reg")[..., 1]) * f(cfg["out_size_factor"])) * f(cfg["voxel_size"][1]) + f(cfg["pc_range"][1])
    z = at("height")[..., 0]
    cols = [x, y, z] + [np.exp(at("dim")[..., k]) for k in range(3)]
    if "vel" in task:
        cols += [at("vel")[..., 0], at("vel")[..., 1]]
    cols.append(np.arctan2(at("rot")[..., 0], at("rot")[..., 1]))
    boxes = np.stack(cols, -1).astype(f).reshape(B, H * W, -1)
    mask = score > f(cfg["score_threshold"])
    r = cfg["post_center_limit_range"]
    if len(r):
        r = np.asarray(r, f)
        mask &= (x >= r[0]) & (y >= r[1]) & (z >= r[2]) & (x <= r[3]) & (y <= r[4]) & (z <= r[5])
    mask = mask.reshape(B, -1)
    out = []
    for b in range(B):
        cell = np.flatnonzero(mask[b])
        out.append((cell, label.reshape(B, -1)[b][cell], boxes[b][cell], score.reshape(B, -1)[b][cell].astype(f)))
    return out


def predict(tasks, cfg, num_classes=HEAD["num_classes"]):
    """the whole post-processing -> per sample (boxes, scores, labels with the tasks' cumulative offset, cells, task)"""
    per_task = [decode(t, cfg) for t in tasks]
    B = len(per_task[0])
    ret = []
    for b in range(B):
        parts, flag = [], 0
        for t, dec in enumerate(per_task):
            cell, label, boxes, score = dec[b]
            if cfg["circular_nms"]:
                keep = nms(boxes, score, "circle", cfg["min_radius"][t], 0, cfg["nms_post_max_size"])
            else:
                keep = nms(boxes, score, "rotate", cfg["nms_iou_threshold"], cfg["nms_pre_max_size"], cfg["nms_post_max_size"],
                           mirror=True)
            parts.append((boxes[keep], score[keep], label[keep] + flag, cell[keep], np.full(keep.size, t)))
            flag += num_classes[t]
        ret.append(tuple(np.concatenate([p[k] for p in parts]) for k in range(5)))
    return ret
