"""Restatement of the first stage's training targets and loss (3dal_pytorch_amd/center_loss.py, rpn.CenterHead.loss;
dal3_center_targets, dal3_center_loss of include/dal3.h) on the CPU, with the seeded inputs of tests/golden/center_loss.npz
(written by tests/golden/gen_center_loss.py from the reference's own AssignLabel, FastFocalLoss, RegLoss and
CenterHead.loss).

`targets` is AssignLabel's train branch in NumPy on the collated (B, G, 10) tensor: the float32 steps (cells, centres) as
float32 operations, the float64 ones (radius, Gaussian) in float64. `loss` is the two criteria, `_sigmoid` and the head's
combination in stock torch ops with autograd, and takes a dtype: float64 is the truth the GPU is judged against (that it
equals the reference's .double() run is what the generator asserts and tests/test_center_loss_cpu.py pins), float32 the
yardstick, the reference's own formulation."""
import numpy as np
import torch

import pillars_ref as P

synth = P.synth
SEED = 20241019
MEASURES, FLOOR, judge, ratios = P.MEASURES, P.FLOOR, P.judge, P.ratios
F64, F32 = torch.float64, torch.float32

# the small cases: a 20 x 24 map (not square: an x / y swap shows) of 0.8 m cells, two tasks of 1 and 2 classes
VOXELS = dict(shape=np.array([192, 160, 40], np.int64), range=np.array([-9.6, -8.0, -3.0, 9.6, 8.0, 3.0], np.float32),
              size=np.array([0.1, 0.1, 0.15], np.float32))
TASKS = [dict(num_class=1, class_names=["VEHICLE"]), dict(num_class=2, class_names=["PEDESTRIAN", "CYCLIST"])]
ASSIGNER = dict(out_size_factor=8, gaussian_overlap=0.1, max_objs=16, min_radius=2, target_assigner=dict(tasks=TASKS))
H, W, G_ROWS = 20, 24, 16
NUM_CLASSES = [1, 2]
HEADS9 = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
HEADS7 = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2))
# (dataset, code_weights, weight, with vel) of the two code sizes, as the reference's nuScenes and Waymo configs have them
CODES = {"c10": ("nuscenes", [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0], 0.25, True),
         "c8": ("waymo", [1.0] * 8, 2.0, False)}
REG_HEADS = ("reg", "height", "dim", "vel", "rot")
CHANNELS = {"reg": 2, "height": 1, "dim": 3, "vel": 2, "rot": 2}
# the mid-size case of the many-block reduction: the first real shape
MID = dict(B=2, H=188, W=188, num_classes=[3], max_objs=500, objects=60, out_size_factor=8,
           voxels=dict(shape=np.array([1504, 1504, 40], np.int64), range=np.array([-75.2, -75.2, -2.0, 75.2, 75.2, 4.0], np.float32),
                       size=np.array([0.1, 0.1, 0.15], np.float32)))

# The GPU tests' bars, by the rule written beside pillars_ref.BARS: multiples of the yardstick (the reference's own fp32
# run against the float64 truth on the same input), the worst ratio recorded on the MI355X (profiles/
# center_loss_measured.json, DAL3_CENTER_LOSS_RECORD over tests/test_gpu_center_loss.py, 128 rows) x at most 2, rounded to
# one significant digit; a bar comes down or stays, it does not go up. Recorded at worst: anno_box 1.00 (every row: the
# kernel's float64 log / sin / cos, rounded once, are never further from float64 than the reference's float32 calls), loss
# 1.02 (main / c8, task 0: both sides carry the float32 clamp constant's 1.8e-5 on log(1 - 0.9999)), grad 1.62 (empty / c8,
# task 0, the heat map: x 2 gives 3.2 -> 3), param_grad 2.88 (tasks.0.hm.1.weight; then 2.43, tasks.0.hm.1.bias: 4 = 1.4 x
# the worst).
BARS = {"anno_box": 2.0, "loss": 2.0, "grad": 3.0, "param_grad": 4.0}


def _row(cx, cy, cls, w=1.3, l=2.1, tag="", vox=VOXELS, osf=8):
    """one GT row whose centre falls at (cx, cy) in cells"""
    u = synth.uniform(SEED, f"center/row/{tag}", (5,))
    cell = np.float64(vox["size"][:2]) * osf
    x, y = np.float64(vox["range"][:2]) + np.array([cx, cy]) * cell
    return [x, y, -1.0 + 2.0 * u[0], w, l, 1.2 + u[1], -3.0 + 6.0 * u[2], -4.0 + 8.0 * u[3], -4.0 + 8.0 * u[4], cls]


def _pack(samples):
    gt = np.zeros((len(samples), G_ROWS, 10), np.float32)
    for b, rows in enumerate(samples):
        for g, r in enumerate(rows):
            if r is not None:
                gt[b, g] = np.asarray(r, np.float64).astype(np.float32)
    return gt


def golden_gt(tag="main"):
    """(2, 16, 10) float32: every case the definition names. None is a padding row (a gap: k differs from the row index)."""
    s0 = [
        _row(3.3, 4.6, 1, 0.9, 1.2, "a0"),              # clamped to min_radius
        _row(0.4, 10.3, 1, 2.0, 4.4, "a1"),             # clipped at the left border
        _row(23.5, 9.2, 1, 2.2, 4.8, "a2"),             # clipped at the right border
        _row(7.5, 7.5, 1, 0.0, 3.0, "a3"),              # w = 0: skipped, its slot stays zero
        _row(-1.7, 5.5, 1, 1.9, 4.1, "a4"),             # out of range, x < 0
        _row(-0.45, 6.4, 1, 2.0, 4.0, "a5"),            # truncates to 0: kept, a negative offset
        _row(np.nan, 3.5, 1, 2.0, 4.0, "a6"),           # a NaN coordinate
        _row(5.5, 1e20, 1, 2.0, 4.0, "a7"),             # beyond int32
        None,
        _row(12.3, 0.6, 2, 2.4, 2.9, "b0"),             # clipped at the top
        _row(8.7, 19.4, 2, 2.6, 3.1, "b1"),             # clipped at the bottom
        _row(11.6, 9.7, 2, 46.0, 50.0, "b2"),           # a radius larger than the map
        _row(15.2, 10.7, 2, 3.1, 3.6, "b3"),            # two overlapping Gaussians of one class
        _row(17.6, 11.3, 2, 3.3, 3.9, "b4"),
        _row(5.5, 15.5, 3, 0.7, 1.9, "b5"),
    ]
    s1 = [
        _row(6.2, 7.3, 1, 2.0, 4.5, "c0"),              # two objects in one cell, the same class
        _row(6.7, 7.8, 1, 1.8, 4.2, "c1"),
        _row(24.3, 4.4, 1, 2.0, 4.0, "c2"),             # out of range, x >= W
        _row(3.3, -2.2, 1, 2.0, 4.0, "c3"),             # y < 0
        _row(4.4, 20.6, 1, 2.0, 4.0, "c4"),             # y >= H
        None,
        _row(10.4, 5.5, 2, 0.8, 0.9, "d0"),             # one cell, two classes
        _row(19.5, 16.5, 2, 0.6, 0.8, "d1"),
        _row(10.6, 5.1, 3, 0.7, 1.8, "d2"),
        _row(14.5, 13.4, 3, 0.8, 2.0, "d3"),
    ]
    if tag == "empty":                                  # task 1 has no object in the whole batch: the num_pos == 0 branch
        s0, s1 = s0[:8], s1[:5]
    else:
        assert tag == "main"
    return _pack([s0, s1])


def mid_gt():
    """(2, 60, 10): 60 objects a sample of 3 classes in class order, anywhere on the 188 x 188 map"""
    m = MID
    gt = np.zeros((m["B"], m["objects"], 10), np.float32)
    for b in range(m["B"]):
        u = synth.uniform(SEED, f"center/mid/{b}", (m["objects"], 4))
        cls = np.sort(1 + (u[:, 0] * 3).astype(np.int64))
        rows = [_row(1.0 + 186.0 * u[i, 1], 1.0 + 186.0 * u[i, 2], cls[i], 0.6 + 2.0 * u[i, 3], 0.8 + 4.5 * u[i, 3], f"mid{b}/{i}",
                     m["voxels"], m["out_size_factor"]) for i in range(m["objects"])]
        gt[b] = np.asarray(rows, np.float64).astype(np.float32)
    return gt


# ------------------------------------------------------------------------------------------------- targets
def _root(a, b, c):
    """what the reference takes for the root of a r^2 - b r + c = 0: (b + sqrt(b^2 - 4 a c)) / 2. The division is by 2
    whatever `a` is: its quirk, kept"""
    return (b + np.sqrt(b * b - 4 * a * c)) / 2


def gaussian_radius(length, width, overlap):
    """the largest centre shift that keeps an IoU of `overlap` with the box, the smallest of three cases: one corner
    moved inward and the other outward, both inward, both outward"""
    side, area = length + width, width * length
    mixed = _root(1, side, area * (1 - overlap) / (1 + overlap))
    inward = _root(4, 2 * side, (1 - overlap) * area)
    outward = _root(4 * overlap, -2 * overlap * side, (overlap - 1) * area)
    return min(mixed, inward, outward)


def cells(gt, voxels, osf):
    """the float32 steps of every row -> (w_c, l_c, ct_x, ct_y), float32 arrays like gt[..., 0]"""
    f = np.float32
    vs, pc, osf = voxels["size"].astype(f), voxels["range"].astype(f), f(osf)
    with np.errstate(all="ignore"):
        return (gt[..., 3] / vs[0] / osf, gt[..., 4] / vs[1] / osf, (gt[..., 0] - pc[0]) / vs[0] / osf, (gt[..., 1] - pc[1]) / vs[1] / osf)


def targets(gt, num_classes, voxels, osf, map_size, overlap=0.1, max_objs=16, min_radius=2, detail=None):
    """-> {'hm': [...], 'anno_box': [...], 'ind': [...], 'mask': [...], 'cat': [...]} per task, NumPy, the reference's
    dtypes, and 'anno_box64': the same rows with log / sin / cos taken in float64 (the truth of those columns).
    detail (a list) receives (b, task, k, radius before int(), ct_x, ct_y) of every object that passed w, l > 0."""
    gt = np.asarray(gt, np.float32)
    B, (Hh, Ww) = gt.shape[0], map_size
    wc, lc, fx, fy = cells(gt, voxels, osf)
    out = {k: [] for k in ("hm", "anno_box", "ind", "mask", "cat", "anno_box64")}
    base = 0
    for t, C in enumerate(num_classes):
        hm = np.zeros((B, C, Hh, Ww), np.float32)
        box, box64 = np.zeros((B, max_objs, 10), np.float32), np.zeros((B, max_objs, 10), np.float64)
        ind, mask, cat = np.zeros((B, max_objs), np.int64), np.zeros((B, max_objs), np.uint8), np.zeros((B, max_objs), np.int64)
        for b in range(B):
            cls = gt[b, :, 9]
            rows = [g for g in range(gt.shape[1]) if base < cls[g] <= base + C]
            for k, g in enumerate(rows[:max_objs]):
                if not (wc[b, g] > 0 and lc[b, g] > 0):
                    continue
                rad = gaussian_radius(np.float64(lc[b, g]), np.float64(wc[b, g]), overlap)
                if detail is not None:
                    detail.append((b, t, k, rad, fx[b, g], fy[b, g]))
                r = max(min_radius, int(rad))
                if not (abs(fx[b, g]) < 2.0 ** 31 and abs(fy[b, g]) < 2.0 ** 31):       # a NaN, an infinity, beyond int32
                    continue
                x, y = int(fx[b, g]), int(fy[b, g])
                if not (0 <= x < Ww and 0 <= y < Hh):
                    continue
                c = int(cls[g]) - 1 - base
                ys, xs = np.arange(max(0, y - r), min(Hh, y + r + 1)), np.arange(max(0, x - r), min(Ww, x + r + 1))
                sigma = (2 * r + 1) / 6
                g2 = np.exp(-((xs[None, :] - x) ** 2.0 + (ys[:, None] - y) ** 2.0) / (2 * sigma * sigma))
                win = hm[b, c, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
                np.maximum(win, g2.astype(np.float32), out=win)
                row = gt[b, g]
                ind[b, k], mask[b, k], cat[b, k] = y * Ww + x, 1, c
                box[b, k] = np.concatenate(([fx[b, g] - np.float32(x), fy[b, g] - np.float32(y), row[2]], np.log(row[3:6]), row[7:9],
                                            [np.sin(row[6]), np.cos(row[6])])).astype(np.float32)
                r64 = row.astype(np.float64)
                box64[b, k] = np.concatenate((box[b, k, :3].astype(np.float64), np.log(r64[3:6]), r64[7:9], [np.sin(r64[6]), np.cos(r64[6])]))
        for k, v in zip(out, (hm, box, ind, mask, cat, box64)):
            out[k].append(v)
        base += C
    return out


# ------------------------------------------------------------------------------------------------- the loss
def _t(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)) if not torch.is_tensor(a) else a
    return t.to(dtype) if dtype is not None and t.is_floating_point() else t


def at_cells(maps, ind):
    """(B, C, H, W) maps read at the flat cells ind (B, M) -> (B, M, C)"""
    flat = maps.flatten(2)
    sample = torch.arange(flat.shape[0], device=flat.device)[:, None]
    return flat[sample, :, ind]


def focal(p, target, ind, mask, cat):
    """the penalty-reduced focal loss on probabilities p: every pixel pays as a negative, damped by (1 - target)^4 near a
    peak; every live slot pays as a positive at its own cell and class; the sum is over the batch's live slots"""
    live = mask.float()
    negatives = ((1 - p).log() * p ** 2 * (1 - target) ** 4).sum()
    peak = at_cells(p, ind).gather(2, cat[:, :, None])
    positives = (peak.log() * (1 - peak) ** 2 * live[:, :, None]).sum()
    count = live.sum()
    total = negatives if count == 0 else (positives + negatives) / count
    return -total


def reg_l1(maps, mask, ind, target):
    """per column: the absolute residuals of the live slots, each over (their number + 1e-4), summed over the batch and
    then over the slots"""
    live = mask.float()[:, :, None]
    residual = (at_cells(maps, ind) * live - target * live).abs() / (live.sum() + 1e-4)
    per_slot = residual.sum(0)                  # (M, C); each column is then summed along its own contiguous row
    return per_slot.t().contiguous().sum(1)


def task_loss(preds, hm_t, box_t, ind, mask, cat, code_weights, weight):
    """one task of the head's loss on raw maps (preds is not changed) -> (loss, hm_loss, loc_loss, loc_loss_elem, num_positive)"""
    hm_loss = focal(torch.sigmoid(preds["hm"]).clamp(1e-4, 1 - 1e-4), hm_t, ind, mask, cat)
    names = [h for h in REG_HEADS if h in preds]
    if "vel" not in preds:                      # the velocity targets have no prediction
        box_t = torch.cat((box_t[..., :6], box_t[..., 8:]), -1)
    elem = reg_l1(torch.cat([preds[h] for h in names], dim=1), mask, ind, box_t)
    loc = (elem * torch.tensor(code_weights, dtype=elem.dtype, device=elem.device)).sum()
    return hm_loss + weight * loc, hm_loss, loc, elem, mask.float().sum()


def loss(preds, tg, code_weights, weight, dtype=F64):
    """preds: per task {head: (B, c, H, W) array}; tg: targets' dictionary -> per task a dict of NumPy arrays: loss, hm_loss,
    loc_loss, loc_loss_elem, num_positive and grad.<head> (autograd's gradient of `loss` in every map)"""
    out = []
    for t, p in enumerate(preds):
        maps = {h: _t(v, dtype).clone().requires_grad_(True) for h, v in p.items()}
        vals = task_loss(maps, _t(tg["hm"][t], dtype), _t(tg["anno_box"][t], dtype), _t(tg["ind"][t]), _t(tg["mask"][t]),
                         _t(tg["cat"][t]), code_weights, weight)
        vals[0].backward()
        r = {k: v.detach().numpy() for k, v in zip(("loss", "hm_loss", "loc_loss", "loc_loss_elem", "num_positive"), vals)}
        r.update({f"grad.{h}": m.grad.numpy() for h, m in maps.items()})
        out.append(r)
    return out


def head_maps(tag, tg, num_classes, with_vel, shape=None, special=True):
    """the seeded raw maps of every task, float32: hm logits around the head's initial bias, and (special) logits large
    enough that both clamps bind (one of them at an object's own pixel), and a height prediction equal to its target,
    which takes the sign(0) path"""
    preds = []
    for t, C in enumerate(num_classes):
        B, _, Hh, Ww = tg["hm"][t].shape if shape is None else shape
        p = {"hm": (-2.19 + 1.5 * synth.normal(SEED, f"center/{tag}/{t}/hm", (B, C, Hh, Ww))).astype(np.float32)}
        for h in REG_HEADS:
            if h != "vel" or with_vel:
                p[h] = synth.normal(SEED, f"center/{tag}/{t}/{h}", (B, CHANNELS[h], Hh, Ww)).astype(np.float32)
        if special:
            flat = p["hm"].reshape(B, C, -1)
            flat[0, 0, 5], flat[0, C - 1, 77], flat[B - 1, 0, 130], flat[B - 1, C - 1, 211] = 12.0, -12.0, 13.5, -14.0
            live = np.argwhere(tg["mask"][t] > 0)
            if len(live):
                (b0, k0), (bm, km), (b1, k1) = live[0], live[len(live) // 2], live[-1]
                flat[b0, tg["cat"][t][b0, k0], tg["ind"][t][b0, k0]] = 12.5
                if len(live) > 2:
                    flat[bm, tg["cat"][t][bm, km], tg["ind"][t][bm, km]] = -12.5
                p["height"].reshape(B, -1)[b1, tg["ind"][t][b1, k1]] = tg["anno_box"][t][b1, k1, 2]
        preds.append(p)
    return preds
