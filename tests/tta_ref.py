"""NumPy restatement of the double-flip test-time augmentation (dal3_flip4_points, dal3_center_decode_flip4 of
include/dal3.h): test infrastructure, built on tests/nms_ref.py, whose seeded head maps and configurations it shares
(tests/golden/gen_tta.py runs the reference on them; the tests rebuild them here).

    flip4_points(points, offsets)   DoubleFlip's views (det3d/datasets/pipelines/test_aug.py), sample b's four consecutive
    merge_decode(task, cfg)         CenterHead.predict with double_flip (center_head.py:318-414) for one task's 4 B maps,
                                    float32 step by step in the reference's order
    predict(tasks, cfg)             the whole post-processing of the merged samples
    mirrored_views(task)            views 1-3 rebuilt from view 0 by the inverse transform (the identity test's input)
"""
import numpy as np

import nms_ref

HEAD = dict(B=8, H=12, W=20, num_classes=nms_ref.HEAD["num_classes"])     # 8 maps: two merged samples; H != W
TOKENS = [f"seq_0_frame_{i}.pkl" for i in range(8)]
RUNS = {"ref_vel": ("ref", True), "ref_novel": ("ref", False), "small_vel": ("small", True), "circle_vel": ("circle", True)}
SWEEP = dict(seed=7, n=37, C=5)                 # DoubleFlip's recorded input


def head_maps(seed, vel=True, **kw):
    return nms_ref.head_maps(seed, vel, **{**{k: v for k, v in HEAD.items()}, **kw})


def sweep():
    rng = np.random.default_rng(SWEEP["seed"])
    pts = rng.normal(0, 20, (SWEEP["n"], SWEEP["C"])).astype(np.float32)
    pts[3, :2] = 0.0                            # signed zeros must come out of the negation as NumPy leaves them
    pts[4, :2] = -0.0
    return pts


def flip4_points(points, offsets):
    """points (N, C) float32, offsets (B + 1) -> out (4 N, C), out_offsets (4 B + 1): view v of sample b at index 4 b + v"""
    points = np.asarray(points, np.float32)
    offsets = np.asarray(offsets, np.int64)
    parts, out_off = [], [4 * int(offsets[0])]
    for b in range(offsets.size - 1):
        rows = points[offsets[b]:offsets[b + 1]]
        for v in range(4):
            p = rows.copy()
            if v & 1:
                p[:, 1] = -p[:, 1]
            if v & 2:
                p[:, 0] = -p[:, 0]
            parts.append(p)
            out_off.append(out_off[-1] + p.shape[0])
    out = np.zeros((4 * points.shape[0], points.shape[1]), np.float32)
    body = np.concatenate(parts) if parts else out[:0]
    out[out_off[0]:out_off[0] + body.shape[0]] = body
    return out, np.asarray(out_off, np.int64)


def mean4(a):
    """a (B, 4, ...) float32 -> torch.mean(dim=1) on the CPU: a running float32 sum in view order, one division"""
    f = np.float32
    return ((((a[:, 0] + a[:, 1]).astype(f) + a[:, 2]).astype(f) + a[:, 3]).astype(f) / f(4)).astype(f)


def _views(task, key):
    """NCHW (4 B, C, H, W) -> (B, 4, H, W, C) float32 with views 1-3 flipped back onto view 0's cells"""
    m = np.transpose(np.asarray(task[key], np.float32), (0, 2, 3, 1))
    m = m.reshape(m.shape[0] // 4, 4, *m.shape[1:]).copy()
    m[:, 1] = m[:, 1, ::-1]
    m[:, 2] = m[:, 2, :, ::-1]
    m[:, 3] = m[:, 3, ::-1, ::-1]
    return m


def _signed(m, one_minus):
    """channel 0 changes under the x-flips (views 2, 3), channel 1 under the y-flips (views 1, 3)"""
    f = np.float32
    m = m.copy()
    for v, c in ((1, 1), (2, 0), (3, 0), (3, 1)):
        m[:, v, ..., c] = (f(1) - m[:, v, ..., c]).astype(f) if one_minus else -m[:, v, ..., c]
    return m


def merge_decode(task, cfg):
    """one task's NCHW maps of 4 B samples -> per MERGED sample (cell (n), label (n), boxes (n, 9 or 7) float32, score (n)
    float32), the survivors in cell order"""
    f = np.float32
    if task["hm"].shape[0] % 4:
        raise ValueError("double_flip needs a batch that is a multiple of 4")
    with np.errstate(over="ignore"):
        sig = mean4((f(1) / (f(1) + np.exp(-_views(task, "hm")))).astype(f))
    B, H, W, _ = sig.shape
    with np.errstate(invalid="ignore"):
        nan = np.isnan(sig)
        label = np.where(nan.any(-1), nan.argmax(-1), sig.argmax(-1))       # torch.max: the first maximum, a NaN wins
        score = np.where(nan.any(-1), f(np.nan), sig.max(-1)).astype(f)
    reg = mean4(_signed(_views(task, "reg"), True))
    ys, xs = np.meshgrid(np.arange(H, dtype=f), np.arange(W, dtype=f), indexing="ij")
    x = ((xs[None] + reg[..., 0]) * f(cfg["out_size_factor"])) * f(cfg["voxel_size"][0]) + f(cfg["pc_range"][0])
    y = ((ys[None] + reg[..., 1]) * f(cfg["out_size_factor"])) * f(cfg["voxel_size"][1]) + f(cfg["pc_range"][1])
    z = mean4(_views(task, "height"))[..., 0]
    dim = mean4(np.exp(_views(task, "dim")).astype(f))
    cols = [x, y, z] + [dim[..., k] for k in range(3)]
    if "vel" in task:
        vel = mean4(_signed(_views(task, "vel"), False))
        cols += [vel[..., 0], vel[..., 1]]
    rot = mean4(_signed(_views(task, "rot"), False))
    cols.append(np.arctan2(rot[..., 0], rot[..., 1]))
    boxes = np.stack(cols, -1).astype(f).reshape(B, H * W, -1)
    with np.errstate(invalid="ignore"):
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
    """-> per merged sample (boxes, scores, labels with the tasks' cumulative offset, cells, task), as nms_ref.predict"""
    per_task = [merge_decode(t, cfg) for t in tasks]
    ret = []
    for b in range(len(per_task[0])):
        parts, flag = [], 0
        for t, dec in enumerate(per_task):
            cell, label, boxes, score = dec[b]
            if cfg["circular_nms"]:
                keep = nms_ref.nms(boxes, score, "circle", cfg["min_radius"][t], 0, cfg["nms_post_max_size"])
            else:
                keep = nms_ref.nms(boxes, score, "rotate", cfg["nms_iou_threshold"], cfg["nms_pre_max_size"],
                                   cfg["nms_post_max_size"], mirror=True)
            parts.append((boxes[keep], score[keep], label[keep] + flag, cell[keep], np.full(keep.size, t)))
            flag += num_classes[t]
        ret.append(tuple(np.concatenate([p[k] for p in parts]) for k in range(5)))
    return ret


def mirrored_views(task):
    """one task's NCHW maps of B samples -> maps of 4 B samples whose views 1-3 are view 0 as the network would see the
    flipped sweep: the maps mirrored, reg -> 1 - reg, rot and vel negated on the flipped axis. With reg a multiple of 2^-10
    every step is exact, so the merge gives view 0 back bit for bit."""
    f = np.float32
    out = {}
    for key, m in task.items():
        m = np.asarray(m, f)
        views = []
        for v in range(4):
            w = m.copy()
            if key in ("reg", "rot", "vel"):
                for c, bit in ((0, 2), (1, 1)):
                    if v & bit:
                        w[:, c] = (f(1) - w[:, c]).astype(f) if key == "reg" else -w[:, c]
            if v & 1:
                w = w[:, :, ::-1]
            if v & 2:
                w = w[:, :, :, ::-1]
            views.append(w)
        out[key] = np.ascontiguousarray(np.stack(views, 1).reshape(4 * m.shape[0], *m.shape[1:]))
    return out
