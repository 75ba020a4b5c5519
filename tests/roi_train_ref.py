"""Restatement of the second stage's training (3dal_pytorch_amd/two_stage.py; dal3_roi_targets, dal3_roi_loss of include/dal3.h)
on the CPU, with the seeded inputs of tests/golden/roi_train.npz (written by tests/golden/gen_roi_train.py from the reference's
own ProposalTargetLayer and RoIHeadTemplate, with the randomness injected as `draws`).

Every step is written once, in torch on the CPU, and takes a dtype: float64 is the truth the GPU is judged against (that it
equals the reference's .double() run is what the generator asserts and tests/test_roi_train_cpu.py pins), float32 the
yardstick, the reference's own formulation in stock fp32 ops. The IoU is tests/iou_ref.py's float64 oracle in both (the
reference's is CUDA-only), rounded to the run's dtype. `fault=` plants one wrong reading of the definition (FAULTS)."""
import numpy as np
import torch
import torch.nn.functional as F

import iou_ref
import roi_ref as R

synth, SEED = R.synth, R.SEED
F64, F32 = R.F64, R.F32
M, ROWS, G = R.GOLDEN_M, 16, 12                 # slots, ROI_PER_IMAGE and GT rows of the golden cases
BIG = dict(M=500, R=128, G=60)                  # the targets-only case at the production sort width
FAULTS = ("fg_strict", "tie_highest", "flip_missing", "pick_unclamped")
TARGET = dict(R.TARGET_CONFIG, ROI_PER_IMAGE=ROWS)
CFG = dict(R.SMALL, TARGET_CONFIG=TARGET)
FLOAT_KEYS = ("gt_iou_of_rois", "rcnn_cls_labels", "gt_of_rois")
THRESHOLDS = (0.1, 0.25, 0.55, 0.75)

# The GPU tests' bars, by the rule written beside pillars_ref.BARS: multiples of the yardstick (the reference's own fp32
# run against its .double() run on the same input), the worst ratio recorded on the MI355X (profiles/
# roi_train_measured.json, DAL3_ROI_TRAIN_RECORD over tests/test_gpu_roi_train.py, 144 rows) x at most 2, rounded up to one
# significant digit, and under a tenth of the smallest planted-fault ratio of tests/test_roi_train_cpu.py; a bar comes down
# or stays, it does not go up. The (B, R) outputs are judged as one column (their columns are no channels). The
# yardstick's overlaps are the float64 oracle's, rounded once (the reference's own IoU is CUDA-only), so the kernel's fp32
# IoU (errors up to 7e-7 absolute) stands many times above it, and the soft labels double that error. Recorded at worst:
# gt_iou_of_rois 11.4 (big: x 2 gives 22.7 -> 30), rcnn_cls_labels 7.20 (c7: 14.4 -> 20), gt_of_rois 1.00 (the kernel's
# arithmetic is the float32 restatement's, operation for operation), the features / rcnn_cls / rcnn_reg 1.23, the
# gradients 2.68 (c7, cls_layers.7.weight), the three losses 4.33 (the one-width head; the bar was set at 8 from c7's
# 3.56 and stays) and the running statistics 2.33 (likewise, 4 from 1.99).
BARS = {"gt_iou_of_rois": 30.0, "rcnn_cls_labels": 20.0, "gt_of_rois": 2.0, "head": 3.0, "grad": 6.0, "loss": 8.0, "stats": 4.0}
SMALLEST_FAULT_RATIO = 3.9e6                    # tie_highest on c7's gt_of_rois (3.95e6, its largest measure); flip_missing 5.27e6


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


# ------------------------------------------------------------------------------------- inputs
def _gt_grid(tag, n, code, nx, pitch, classes):
    """n separated GT rows (code + 1 columns) on a grid of `pitch` metres: no two overlap"""
    ix = np.arange(n)
    xy = np.stack([(ix % nx - (nx - 1) / 2) * pitch[0], (ix // nx - 1) * pitch[1]], 1) + synth.uniform(SEED, f"{tag}/j", (n, 2), -0.1, 0.1)
    z = synth.uniform(SEED, f"{tag}/z", (n, 1), -0.5, 0.5)
    dims = synth.uniform(SEED, f"{tag}/d", (n, 3), 0.0, 1.0) * [0.6, 0.3, 0.4] + [0.8, 0.4, 0.8]
    rot = synth.uniform(SEED, f"{tag}/r", (n, 1), -np.pi, np.pi)
    vel = synth.uniform(SEED, f"{tag}/v", (n, 2), -3.0, 3.0)
    cls = np.asarray(classes, np.float64)[ix % len(classes)][:, None]
    return np.concatenate([xy, z, dims, rot] + ([vel] if code == 9 else []) + [cls], 1).astype(np.float32)


def _roi_near(tag, gt_row, target, code):
    """a RoI (rotation at column 6) whose IoU with gt_row is `target` within 0.02 and 2e-3 away from every threshold: the GT
    box with its size and heading disturbed (half of them turned by pi: both sides of the flip), shifted along a seeded
    direction by bisection"""
    u = synth.uniform(SEED, tag, (8,))
    box = gt_row[:7].astype(np.float64).copy()
    box[3:6] *= 1.0 + (u[0:3] - 0.5) * 0.04
    box[6] += (u[3] - 0.5) * 0.06 + (np.pi if u[4] < 0.5 else 0.0) + (2 * np.pi if u[5] < 0.25 else 0.0)
    phi = u[6] * 2 * np.pi
    direction = np.asarray([np.cos(phi), np.sin(phi), 0.3 * (u[7] - 0.5)])
    lo, hi = 0.0, 3.0

    def at(s):
        b = box.copy()
        b[:3] += s * direction
        b = b.astype(np.float32)
        return b, float(iou_ref.paired(b[None], gt_row[None, :7])[1][0])
    assert at(0.0)[1] > target, (tag, at(0.0)[1], target)
    for _ in range(40):
        mid = (lo + hi) / 2
        b, v = at(mid)
        if abs(v - target) < 0.02 and min(abs(v - t) for t in THRESHOLDS) > 2e-3:
            break
        lo, hi = (mid, hi) if v > target else (lo, mid)
    else:
        raise AssertionError(f"no shift gives IoU {target} for {tag}")
    vel = gt_row[7:9] + (u[0:2] - 0.5) if code == 9 else np.zeros(0)
    return np.concatenate([b, vel]).astype(np.float32)


def _sample(tag, code, gt, plan, n_slots=M, n_gt=G):
    """plan: [(gt row or None, target IoU, label or None for the row's class)] for the live slots -> rois (n_slots, code), scores,
    labels (int64; 0: an empty slot), gt (n_gt, code + 1)"""
    rois, labels = np.zeros((n_slots, code), np.float32), np.zeros(n_slots, np.int64)
    for i, (g, target, label) in enumerate(plan):
        if g is None:                           # far from every GT
            far = R.boxes(f"{tag}/far{i}", 1, code)[0]
            far = far[[0, 1, 2, 3, 4, 5, 8, 6, 7]] if code == 9 else far
            far[:2] += 40.0
            rois[i], labels[i] = far, label
        else:
            rois[i] = _roi_near(f"{tag}/roi{i}", gt[g], target, code)
            labels[i] = int(gt[g][-1]) if label is None else label
    scores = np.zeros(n_slots, np.float32)
    scores[:len(plan)] = synth.uniform(SEED, f"{tag}/s", (len(plan),), 0.1, 0.95)
    full = np.zeros((n_gt, code + 1), np.float32)
    full[:gt.shape[0]] = gt
    return rois, scores, labels, full


def _spread(lo, hi, n):
    return list(np.linspace(lo, hi, n))


def golden_inputs(code):
    """the two samples of golden case c7 / c9 -> rois (2, M, code), roi_scores, roi_labels, gt_boxes_and_cls (2, G, code + 1),
    draws (2, M + ROWS). c7: sample 0 fg and bg (12 fg > ROWS / 2, 3 hard bg < the cap of 6, easy bg, a class without GT,
    two interior zero GT rows, trailing zero rows, 8 empty slots), sample 1 fg only (48 slots above 0.55). c9: sample 0 fg
    and hard-only bg (5 fg, 43 hard, no slot empty), sample 1 bg only without GT (easy only)."""
    tag = f"t{code}"
    if code == 7:
        g0 = _gt_grid(f"{tag}/g0", 9, code, 3, (2.2, 1.8), (1, 2))
        g0[3] = 0                               # interior zero rows: class 0, met by the empty slots
        g0[5] = 0
        live = [0, 1, 2, 4, 6, 7, 8]
        plan = [(live[i % 7], v, None) for i, v in enumerate(_spread(0.6, 0.88, 12))]
        plan += [(live[i], v, None) for i, v in enumerate((0.15, 0.3, 0.45))]
        plan += [(live[i % 7], 0.04, None) for i in range(6)] + [(None, 0, 1 + i % 2) for i in range(13)]
        plan += [(live[i], 0.8, 3) for i in range(6)]                        # class 3 has no GT: overlap 0
        order = np.argsort(synth.uniform(SEED, f"{tag}/order0", (len(plan),)))
        s0 = _sample(f"{tag}/s0", code, g0, [plan[i] for i in order])
        g1 = _gt_grid(f"{tag}/g1", 6, code, 3, (2.2, 1.8), (1, 2, 3))
        s1 = _sample(f"{tag}/s1", code, g1, [(i % 6, v, None) for i, v in enumerate(_spread(0.6, 0.88, M))])
    else:
        g0 = _gt_grid(f"{tag}/g0", 8, code, 4, (2.0, 1.8), (1, 2, 3))
        plan = [(i, v, None) for i, v in enumerate(_spread(0.62, 0.88, 5))] + [(i % 8, v, None) for i, v in enumerate(_spread(0.13, 0.52, 43))]
        order = np.argsort(synth.uniform(SEED, f"{tag}/order0", (len(plan),)))
        s0 = _sample(f"{tag}/s0", code, g0, [plan[i] for i in order])
        s1 = _sample(f"{tag}/s1", code, np.zeros((1, code + 1), np.float32), [(None, 0, 1 + i % 3) for i in range(23)])
    draws = synth.uniform(SEED, f"{tag}/draws", (2, M + ROWS)).astype(np.float32)
    assert draws.max() < 1.0
    rois, scores, labels, gt = (np.stack(v) for v in zip(s0, s1))
    return dict(rois=rois, roi_scores=scores, roi_labels=labels, gt_boxes_and_cls=gt, draws=draws)


def big_inputs():
    """the targets-only case: one sample of 500 slots (430 live: 150 fg, 100 hard, far and low ones), 60 GT rows, 128 rows"""
    m, g = BIG["M"], BIG["G"]
    gt = _gt_grid("big/g", g - 4, 9, 8, (2.2, 1.8), (1, 2, 3))
    plan = [(i % 56, v, None) for i, v in enumerate(_spread(0.58, 0.88, 150))] + [(i % 56, v, None) for i, v in enumerate(_spread(0.12, 0.53, 100))]
    plan += [(i % 56, 0.05, None) for i in range(60)] + [(None, 0, 1 + i % 3) for i in range(120)]
    order = np.argsort(synth.uniform(SEED, "big/order", (len(plan),)))
    rois, scores, labels, full = _sample("big/s2", 9, gt, [plan[i] for i in order], m, g)
    draws = synth.uniform(SEED, "big/draws", (1, m + BIG["R"])).astype(np.float32)
    return dict(rois=rois[None], roi_scores=scores[None], roi_labels=labels[None], gt_boxes_and_cls=full[None], draws=draws)


def drop_masks(cfg, rows, tag):
    """the multipliers of the head's Dropout modules in the order they run (shared, cls, reg): 0 or 1 / (1 - p)"""
    p = cfg["DP_RATIO"]
    widths = [w for w in cfg["SHARED_FC"][:-1]] + [cfg["CLS_FC"][0], cfg["REG_FC"][0]]
    return [((synth.uniform(SEED, f"{tag}/drop{i}", (rows, w)) >= p) / (1.0 - p)).astype(np.float32) for i, w in enumerate(widths)]


# ------------------------------------------------------------------------------------- the target assignment
def iou3d(rois7, gt7, dtype):
    """the reference's boxes_iou3d_gpu by the float64 oracle, rounded to the run's dtype. Its union is clamped at 1e-6; the
    oracle returns 0 for an empty union, which is the same number for the boxes of these cases (asserted)."""
    a, b = np.asarray(rois7, np.float64), np.asarray(gt7, np.float64)
    va, vb = a[:, 3] * a[:, 4] * a[:, 5], b[:, 3] * b[:, 4] * b[:, 5]
    union = va[:, None] + vb[None, :]
    assert ((union == 0) | (union > 1e-3)).all()
    return _t(iou_ref.pairwise(a, b)[1], dtype)


def max_iou_same_class(rois, labels, gt, dtype, fault=None):
    """get_max_iou_with_same_class as one rule: the maximum over the GT rows of the RoI's class, the lowest such row among
    the maxima, (0, 0) without one"""
    iou = iou3d(rois[:, :7], gt[:, :7], dtype)
    same = labels[:, None] == gt[:, -1].long()[None, :]
    masked = torch.where(same, iou, torch.full_like(iou, -1.0))
    best = masked.max(1).values
    hit = same & (masked == best[:, None])
    idx = torch.arange(gt.shape[0])
    asg = torch.where(hit, idx, torch.full_like(idx, -1 if fault == "tie_highest" else gt.shape[0]))
    asg = asg.max(1).values if fault == "tie_highest" else asg.min(1).values
    none = ~same.any(1)
    return torch.where(none, torch.zeros_like(best), best), torch.where(none, torch.zeros_like(asg), asg)


def draw(pick, n, fault=None):
    """the with-replacement draws: min(int(pick * n), n - 1), the product a float32 one"""
    i = (np.asarray(pick, np.float32) * np.float32(n)).astype(np.int64)
    return i if fault == "pick_unclamped" else np.minimum(i, n - 1)


def subsample(overlaps, cfg, key, pick, fault=None):
    """subsample_rois / sample_bg_inds with the randomness given: key orders the fg positions, pick[c] draws background
    row c (or, fg only, row c) -> sampled slots (ROI_PER_IMAGE)"""
    rows = cfg["ROI_PER_IMAGE"]
    fg_per_image = int(np.round(cfg["FG_RATIO"] * rows))
    fg_thresh = min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"])
    o = overlaps
    fg = ((o > fg_thresh) if fault == "fg_strict" else (o >= fg_thresh)).nonzero().view(-1).numpy()
    easy = (o < cfg["CLS_BG_THRESH_LO"]).nonzero().view(-1).numpy()
    hard = ((o < cfg["REG_FG_THRESH"]) & (o >= cfg["CLS_BG_THRESH_LO"])).nonzero().view(-1).numpy()

    def background(n):
        p = np.asarray(pick[:n])
        if len(hard) and len(easy):
            hn = min(int(n * cfg["HARD_BG_RATIO"]), len(hard))
            return np.concatenate([hard[draw(p[:hn], len(hard), fault)], easy[draw(p[hn:], len(easy), fault)]])
        both = hard if len(hard) else easy
        return both[draw(p, len(both), fault)]
    if len(fg) and len(hard) + len(easy):
        n = min(fg_per_image, len(fg))
        perm = np.argsort(np.asarray(key[:len(fg)]), kind="stable")
        return np.concatenate([fg[perm[:n]], background(rows - n)])
    if len(fg):
        return fg[draw(pick[:rows], len(fg), fault)]
    if len(hard) + len(easy):
        return background(rows)
    raise NotImplementedError("neither fg nor bg")


def limit_period(val, offset, period):
    return val - torch.floor(val / period + offset) * period


def targets(inp, cfg, dtype=F64, fault=None):
    """ProposalTargetLayer.forward + assign_targets -> the reference's targets_dict (without roi_features) plus `slot`
    (B, ROI_PER_IMAGE) and `sample` (b, or -1 for an empty slot)"""
    rois_all, scores_all = _t(inp["rois"], dtype), _t(inp["roi_scores"], dtype)
    labels_all, gt_all, draws = torch.as_tensor(inp["roi_labels"]).long(), _t(inp["gt_boxes_and_cls"], dtype), np.asarray(inp["draws"])
    B, n_slots, code = rois_all.shape
    rows = cfg["ROI_PER_IMAGE"]
    out = {k: [] for k in ("slot", "sample", "rois", "roi_labels", "roi_scores", "gt_iou_of_rois", "gt_of_rois_src")}
    for b in range(B):
        gt = gt_all[b]
        k = gt.shape[0] - 1
        while k > 0 and gt[k].sum() == 0:
            k -= 1
        gt = gt[:k + 1]
        overlaps, asg = max_iou_same_class(rois_all[b], labels_all[b], gt, dtype, fault)
        s = torch.as_tensor(subsample(overlaps, cfg, draws[b, :n_slots], draws[b, n_slots:], fault))
        out["slot"].append(s)
        out["sample"].append(torch.where(labels_all[b][s] != 0, b, -1))
        out["rois"].append(rois_all[b][s])
        out["roi_labels"].append(labels_all[b][s])
        out["roi_scores"].append(scores_all[b][s])
        out["gt_iou_of_rois"].append(overlaps[s])
        out["gt_of_rois_src"].append(gt[asg[s]])
    out = {k: torch.stack(v) for k, v in out.items()}
    iou = out["gt_iou_of_rois"]
    out["reg_valid_mask"] = (iou > cfg["REG_FG_THRESH"]).long()
    fg_t, bg_t = cfg["CLS_FG_THRESH"], cfg["CLS_BG_THRESH"]
    if cfg["CLS_SCORE_TYPE"] == "cls":
        lab = (iou > fg_t).long()
        lab[(iou > bg_t) & (iou < fg_t)] = -1
    else:
        fg_mask, bg_mask = iou > fg_t, iou < bg_t
        interval = (~fg_mask) & (~bg_mask)
        lab = fg_mask.to(dtype)
        lab[interval] = (iou[interval] - bg_t) / (fg_t - bg_t)
    out["rcnn_cls_labels"] = lab
    rois, g = out["rois"], out["gt_of_rois_src"].clone()
    ry = limit_period(rois[:, :, 6], 0.5, np.pi * 2)
    g[:, :, :6] = g[:, :, :6] - rois[:, :, :6]
    g[:, :, 6] = g[:, :, 6] - ry
    c, s = torch.cos(-ry), torch.sin(-ry)
    x, y = g[:, :, 0] * c + g[:, :, 1] * s, g[:, :, 0] * (-s) + g[:, :, 1] * c
    g[:, :, 0], g[:, :, 1] = x, y
    if code == 9:
        g[:, :, 7:-1] = g[:, :, 7:-1] - rois[:, :, 7:]
    h = g[:, :, 6] % (2 * np.pi)
    if fault != "flip_missing":
        opposite = (h > np.pi * 0.5) & (h < np.pi * 1.5)
        h[opposite] = (h[opposite] + np.pi) % (2 * np.pi)
    flag = h > np.pi
    h[flag] = h[flag] - np.pi * 2
    g[:, :, 6] = torch.clamp(h, min=-np.pi / 2, max=np.pi / 2)
    out["gt_of_rois"] = g
    return out


# ------------------------------------------------------------------------------------- the head in train mode and the losses
def head_params(sd, dtype):
    """leaf tensors of the head's parameters and copies of its running statistics"""
    params = {k: _t(v, dtype).requires_grad_(True) for k, v in sd.items() if "running" not in k and "num_batches" not in k}
    stats = {k: _t(v, dtype).clone() for k, v in sd.items() if "running" in k}
    return params, stats


def train_mlp(params, stats, cfg, feats, masks, eps=1e-5, momentum=0.1):
    """the three Sequential stacks in train mode on (N, c_in) rows: batch statistics over the N rows, running statistics
    updated in `stats`, the Dropout multipliers given -> rcnn_cls (N, 1), rcnn_reg (N, code)"""
    masks = list(masks)
    x = feats.unsqueeze(-1)
    outs, shared = {}, None
    n_shared = len(cfg["SHARED_FC"])
    k_in = {"shared": 0, "cls": 0, "reg": 0}
    for conv, bn, _ in R.layer_names(cfg):
        part = conv.split("_")[0]
        if conv.endswith(".0.") and part != "shared":
            if shared is None:
                shared = x
            x = shared
        bias = params.get(conv + "bias")
        x = F.conv1d(x, params[conv + "weight"], bias)
        if bn is None:
            outs[part] = x.squeeze(-1)
            continue
        x = F.relu(F.batch_norm(x, stats[bn + "running_mean"], stats[bn + "running_var"], params[bn + "weight"], params[bn + "bias"],
                                True, momentum, eps))
        k = k_in[part]
        k_in[part] += 1
        if (part == "shared" and k != n_shared - 1 and cfg["DP_RATIO"] > 0) or (part != "shared" and k == 0 and cfg["DP_RATIO"] >= 0):
            x = x * _t(masks.pop(0), x.dtype).unsqueeze(-1)
    assert not masks
    return outs["cls"], outs["reg"]


def losses(rcnn_cls, rcnn_reg, tg, loss_cfg):
    """get_box_cls_layer_loss (BinaryCrossEntropy) + get_box_reg_layer_loss (L1) -> (cls, reg, total)"""
    code = rcnn_reg.shape[-1]
    w = loss_cfg["LOSS_WEIGHTS"]
    lab = tg["rcnn_cls_labels"].view(-1)
    p = torch.sigmoid(rcnn_cls.view(-1))
    y = lab.to(p.dtype)
    each = -(y * torch.clamp(torch.log(p), min=-100.0) + (1 - y) * torch.clamp(torch.log(1 - p), min=-100.0))
    valid = (lab >= 0).to(p.dtype)
    cls = (each * valid).sum() / torch.clamp(valid.sum(), min=1.0) * w["rcnn_cls_weight"]
    fg = tg["reg_valid_mask"].view(-1) > 0
    fg_sum = int(fg.long().sum())
    diff = (rcnn_reg - tg["gt_of_rois"][..., :code].reshape(-1, code)).abs() * rcnn_reg.new_tensor(w["code_weights"][:code])
    reg = (diff * fg.unsqueeze(-1).to(p.dtype)).sum() / max(fg_sum, 1) * w["rcnn_reg_weight"]
    return cls, reg, cls + reg


def gather_features(bev, tg, num_point=R.NUM_POINT, dtype=F64):
    """the feature rows of the sampled RoIs: roi_ref's gather at the sampled boxes, zero rows for the empty slots"""
    B, rows, code = tg["rois"].shape
    out = []
    for b in range(B):
        box = tg["rois"][b].to(dtype)
        box = box[:, [0, 1, 2, 3, 4, 5, 7, 8, 6]] if code == 9 else box
        f = R.bev_features(bev[b:b + 1], [R.box_points(box, num_point, dtype)], num_point, dtype=dtype)[0]
        out.append(f * (tg["sample"][b] >= 0).to(dtype)[:, None])
    return torch.stack(out)


def run(sd, cfg, bev, inp, masks, dtype=F64, fault=None):
    """the reference's forward(training=True) + get_loss + backward on the golden inputs -> a dict: the targets, features,
    rcnn_cls, rcnn_reg, loss (3), d_cls, d_reg, grads {key: gradient}, stats {key: updated running statistic}"""
    with torch.enable_grad():                   # whatever the caller (or a test before it) left switched
        tg = targets(inp, cfg["TARGET_CONFIG"], dtype, fault)
        feats = gather_features(bev, tg, dtype=dtype)
        params, stats = head_params(sd, dtype)
        cls, reg = train_mlp(params, stats, cfg, feats.view(-1, feats.shape[-1]), masks)
        cls.retain_grad()
        reg.retain_grad()
        l_cls, l_reg, total = losses(cls, reg, tg, cfg["LOSS_CONFIG"])
        total.backward()
    return dict(tg, features=feats, rcnn_cls=cls.detach(), rcnn_reg=reg.detach(), loss=torch.stack([l_cls, l_reg, total]).detach(),
                d_cls=cls.grad, d_reg=reg.grad, grads={k: v.grad for k, v in params.items()}, stats=stats)


def golden_case(code):
    base = R.golden_case(code)
    inp = golden_inputs(code)
    return dict(sd=base["sd"], cfg=dict(CFG), bev=base["bev"], inp=inp, masks=drop_masks(CFG, 2 * ROWS, f"t{code}"))


def stability(tg64):
    """the conditions under which float32 rounding cannot move a discrete decision (the issue's list); overlaps part"""
    iou = tg64["gt_iou_of_rois"].numpy()
    return min(float(np.abs(iou - t).min()) for t in THRESHOLDS)
