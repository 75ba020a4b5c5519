"""Restatements of CenterPoint's second stage (3dal_pytorch_amd/two_stage.py; dal3_bev_gather, dal3_box_points, dal3_roi_pack,
dal3_roi_head, dal3_roi_post of include/dal3.h) on the CPU, with the seeded inputs and weights of tests/golden/roi.npz
(written by tests/golden/gen_roi.py from the reference's own BEVFeatureExtractor, RoIHead and TwoStageDetector methods).

Every step is written once, in torch on the CPU, from the UNFOLDED parameters, and takes a dtype: in float64 it is the
truth the GPU is judged against (that it equals the reference's .double() outputs is what tests/test_roi_cpu.py pins); in
float32 it is the yardstick, the reference's own formulation in stock fp32 ops. `fold` is the packing's arithmetic bit for
bit. `fault=` plants one wrong reading of the definition at a time (FAULTS). The measures are pillars_ref.judge's."""
import numpy as np
import torch
import torch.nn.functional as F

import fold_ref
import pillars_ref as P

synth = P.synth
SEED = 20241019
MEASURES, FLOOR, judge, ratios = P.MEASURES, P.FLOOR, P.judge, P.ratios
F64, F32 = torch.float64, torch.float32

TARGET_CONFIG = dict(ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75,
                     CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
LOSS_CONFIG = dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="L1",
                   LOSS_WEIGHTS={"rcnn_cls_weight": 1.0, "rcnn_reg_weight": 1.0, "code_weights": [1.0] * 7 + [0.2, 0.2]})


def model_cfg(shared, cls, reg, dp=0.3):
    return dict(CLASS_AGNOSTIC=True, SHARED_FC=list(shared), CLS_FC=list(cls), REG_FC=list(reg), DP_RATIO=dp,
                TARGET_CONFIG=TARGET_CONFIG, LOSS_CONFIG=LOSS_CONFIG)


SMALL = model_cfg([32, 32], [16, 48], [16, 48])             # 100 inputs: a K tail, widths that differ
PRODUCTION = model_cfg([256, 256], [256, 256], [256, 256])  # 2560 inputs
# the golden map: B = 2, 6 x 9 cells (not square), C = 20; the extractor's geometry
MAP = dict(B=2, H=6, W=9, C=20)
EXTRACTOR = dict(pc_start=[-3.6, -2.4], voxel_size=[0.1, 0.1], out_stride=8)       # a cell is 0.8 m: x in [-3.6, 3.6], y in [-2.4, 2.4]
NUM_POINT = 5
GOLDEN_M = 48                                   # NMS_POST_MAXSIZE of the golden run
GOLDEN_BOXES = (40, 23)                         # kept boxes per sample
FAULTS = ("xy_swapped", "hw_swapped", "weights_unclamped", "sections_interleaved", "front_back_swapped", "rot_column_6",
          "eps_1e-3", "velocity_rotated", "sqrt_dropped", "labels_not_shifted")

# The GPU tests' bars: multiples of the yardstick (the float32 restatement's own error against the float64 truth on the
# same input), by the rule written beside pillars_ref.BARS: the worst ratio of the first MI355X run
# (profiles/roi_measured.json, DAL3_ROI_RECORD over tests/test_gpu_roi.py and tests/test_gpu_two_stage.py) x at most 2,
# rounded up to one significant digit, and under a tenth of the smallest planted-fault ratio of tests/test_roi_cpu.py
# (SMALLEST_FAULT_RATIO below); a bar comes down or stays, it does not go up. That run (28 rows: the gather at C = 1, 20 and
# 64 through both layouts, RoIHead at 37 and 500 rows for both code sizes and at the production widths, both golden cases
# stage by stage) recorded at worst tensor 1.26 (head/cls/m500/c9), chan_rms 1.20 (golden/c7/cls) and chan_max 1.58
# (head/box/m37/c9): x 2 gives 2.5 -> 3 and 2.4 -> 3, x 1.9 gives 3. The gather's rows are 1.00 throughout (its arithmetic
# is the float32 restatement's, operation for operation, and so are its bits: on the lines, below them, and at +-1e6 m).
BARS = {"tensor": 3.0, "chan_rms": 3.0, "chan_max": 3.0}
SMALLEST_FAULT_RATIO = 3.0e3                    # eps_1e-3 on c7's box_preds (3.03e3, its largest measure); every other fault > 1e6


def bev_map(tag="map", B=MAP["B"], H=MAP["H"], W=MAP["W"], C=MAP["C"]):
    """(B, H, W, C) float32, post-ReLU-like: non-negative, a fifth of the entries +0"""
    x = synth.uniform(SEED, f"{tag}/x", (B, H, W, C), -0.5, 2.0)
    return np.maximum(x, 0.0).astype(np.float32)


def boxes(tag, n, cols, spread=1.0):
    """n first-stage boxes [x, y, z, dx, dy, dz, (vx, vy), rot]: centres inside the golden map and beyond every side of it
    (spread 1: about a third outside), headings beyond +-pi"""
    lo = np.asarray(EXTRACTOR["pc_start"])
    ext = np.asarray([MAP["W"], MAP["H"]]) * 0.8
    xy = lo + ext * synth.uniform(SEED, f"{tag}/xy", (n, 2), 0.5 - 0.75 * spread, 0.5 + 0.75 * spread)
    z = synth.uniform(SEED, f"{tag}/z", (n, 1), -1.0, 1.0)
    dims = synth.uniform(SEED, f"{tag}/d", (n, 3), 0.4, 2.5)
    vel = synth.uniform(SEED, f"{tag}/v", (n, 2), -5.0, 5.0)
    rot = synth.uniform(SEED, f"{tag}/r", (n, 1), -2.0 * np.pi, 2.0 * np.pi)
    parts = [xy, z, dims] + ([vel] if cols == 9 else []) + [rot]
    return np.concatenate(parts, 1).astype(np.float32)


def first_pred(tag, cols, counts=GOLDEN_BOXES):
    """the first stage's per-sample list: box3d_lidar, scores in (0, 1), label_preds in {0, 1, 2}"""
    out = []
    for i, n in enumerate(counts):
        out.append({"box3d_lidar": boxes(f"{tag}/{i}", n, cols),
                    "scores": synth.uniform(SEED, f"{tag}/{i}/s", (n,), 0.1, 0.95).astype(np.float32),
                    "label_preds": (synth.uniform(SEED, f"{tag}/{i}/l", (n,), 0, 3).astype(np.int64) % 3)})
    return out


# ------------------------------------------------------------------------------------- weights
def layer_names(cfg):
    """[(prefix of the conv, prefix of its BatchNorm or None, c_out or None for a final layer)] with the reference's
    Sequential indices (the Dropout slots included), in dal3_roi_pack's order"""
    dp, out = cfg["DP_RATIO"], []
    i = 0
    for k, w in enumerate(cfg["SHARED_FC"]):
        out.append((f"shared_fc_layer.{i}.", f"shared_fc_layer.{i + 1}.", w))
        i += 3 + (1 if k != len(cfg["SHARED_FC"]) - 1 and dp > 0 else 0)
    for name, key in (("cls_layers", "CLS_FC"), ("reg_layers", "REG_FC")):
        i = 0
        for k, w in enumerate(cfg[key]):
            out.append((f"{name}.{i}.", f"{name}.{i + 1}.", w))
            i += 3 + (1 if dp >= 0 and k == 0 else 0)
        out.append((f"{name}.{i}.", None, None))
    return out


def head_weights(input_channels, cfg, code_size, tag="roi"):
    """a reference-keyed state_dict of RoIHead: seeded uniform weights scaled by fan-in (mean-free over the fan-in, as
    rpn_ref._w has them: the inputs are non-negative), BatchNorm statistics away from (0, 1)"""
    sd, shared_out = {}, cfg["SHARED_FC"][-1]
    pre = input_channels
    for conv, bn, w in layer_names(cfg):
        if conv.endswith(".0.") and not conv.startswith("shared"):
            pre = shared_out
        final = bn is None
        c_out = (1 if conv.startswith("cls") else code_size) if final else w
        a = np.sqrt(6.0 / pre)
        wt = synth.uniform(SEED, f"{tag}/{conv}w", (c_out, pre, 1), -a, a)
        sd[conv + "weight"] = (wt - wt.mean(axis=1, keepdims=True)).astype(np.float32)
        if final:
            sd[conv + "bias"] = synth.uniform(SEED, f"{tag}/{conv}b", (c_out,), -0.5, 0.5).astype(np.float32)
        else:
            sd[bn + "weight"] = synth.uniform(SEED, f"{tag}/{bn}g", (c_out,), 0.5, 1.5).astype(np.float32)
            sd[bn + "bias"] = synth.uniform(SEED, f"{tag}/{bn}b", (c_out,), 0.1, 0.5).astype(np.float32)
            sd[bn + "running_mean"] = synth.uniform(SEED, f"{tag}/{bn}m", (c_out,), -0.3, 0.3).astype(np.float32)
            sd[bn + "running_var"] = synth.uniform(SEED, f"{tag}/{bn}v", (c_out,), 0.5, 2.0).astype(np.float32)
            sd[bn + "num_batches_tracked"] = np.asarray(7, np.int64)
        pre = c_out
    return sd


def fold(w, bias, bn, eps):
    """fold_ref.fold with a Conv1d's weight as (c_out, c_in)"""
    return fold_ref.fold(np.asarray(w).reshape(np.shape(w)[0], -1), bias, bn, eps, 0)


def bn_of(sd, p):
    return tuple(sd[p + k] for k in ("weight", "bias", "running_mean", "running_var"))


# ------------------------------------------------------------------------------------- the steps
def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def box_points(box, num_point, dtype=F64, fault=None):
    """get_box_center for one sample: (n, cols) -> (num_point * n, 3), sections one after another"""
    box = _t(box, dtype)
    if num_point == 1 or box.shape[0] == 0:
        return box[:, :3]
    centre, height, dims = box[:, :2], box[:, 2:3], box[:, 3:5]
    rot = box[:, 6] if fault == "rot_column_6" else box[:, -1]
    norm = torch.tensor([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]], dtype=dtype)
    corners = dims.view(-1, 1, 2) * norm.view(1, 4, 2)
    s, c = torch.sin(rot), torch.cos(rot)
    rot_t = torch.stack([torch.stack([c, -s]), torch.stack([s, c])])
    corners = torch.einsum("aij,jka->aik", corners, rot_t) + centre.view(-1, 1, 2)
    front, back = (corners[:, 0] + corners[:, 1]) / 2, (corners[:, 2] + corners[:, 3]) / 2
    left, right = (corners[:, 0] + corners[:, 3]) / 2, (corners[:, 1] + corners[:, 2]) / 2
    if fault == "front_back_swapped":
        front, back = back, front
    return torch.cat([box[:, :3]] + [torch.cat([m, height], -1) for m in (front, back, left, right)], 0)


def relative(points, ext=EXTRACTOR, dtype=F64):
    """absl_to_relative: three operations in this order, the Python scalars at the tensor's precision"""
    points = _t(points, dtype)
    x = (points[..., 0] - ext["pc_start"][0]) / ext["voxel_size"][0] / ext["out_stride"]
    y = (points[..., 1] - ext["pc_start"][1]) / ext["voxel_size"][1] / ext["out_stride"]
    return x, y


def bilinear(im, x, y, fault=None):
    """bilinear_interpolate_torch: im (H, W, C), x / y (n) relative coordinates of im's dtype"""
    if fault == "xy_swapped":
        x, y = y, x
    H, W = (im.shape[1], im.shape[0]) if fault == "hw_swapped" else (im.shape[0], im.shape[1])
    x0, y0 = torch.floor(x).long(), torch.floor(y).long()
    x1, y1 = x0 + 1, y0 + 1
    ux1, uy1 = x1, y1
    x0, x1 = torch.clamp(x0, 0, W - 1), torch.clamp(x1, 0, W - 1)
    y0, y1 = torch.clamp(y0, 0, H - 1), torch.clamp(y1, 0, H - 1)
    if fault == "hw_swapped":                   # the wrong clamp, then whatever still indexes
        x0, x1 = x0.clamp(max=im.shape[1] - 1), x1.clamp(max=im.shape[1] - 1)
        y0, y1 = y0.clamp(max=im.shape[0] - 1), y1.clamp(max=im.shape[0] - 1)
    if fault != "weights_unclamped":
        ux1, uy1 = x1, y1
    Ia, Ib, Ic, Id = im[y0, x0], im[y1, x0], im[y0, x1], im[y1, x1]
    wa = (ux1.type_as(x) - x) * (uy1.type_as(y) - y)
    wb = (ux1.type_as(x) - x) * (y - y0.type_as(y))
    wc = (x - x0.type_as(x)) * (uy1.type_as(y) - y)
    wd = (x - x0.type_as(x)) * (y - y0.type_as(y))
    return torch.t(torch.t(Ia) * wa) + torch.t(torch.t(Ib) * wb) + torch.t(torch.t(Ic) * wc) + torch.t(torch.t(Id) * wd)


def bev_features(bev, centres, num_point, ext=EXTRACTOR, dtype=F64, fault=None):
    """BEVFeatureExtractor.forward: bev (B, H, W, C), centres[b] (num_point * n_b, 3) -> [(n_b, num_point * C)]"""
    bev = _t(bev, dtype)
    out = []
    for b in range(bev.shape[0]):
        x, y = relative(centres[b], ext, dtype)
        f = bilinear(bev[b], x, y, fault)
        if num_point > 1:
            n = f.shape[0] // num_point
            if fault == "sections_interleaved":
                f = f.view(num_point, n, -1).permute(1, 2, 0).reshape(n, -1)
            else:
                f = torch.cat([f[i * n:(i + 1) * n] for i in range(num_point)], 1)
        out.append(f)
    return out


def reorder(pred, feats, M, code_size, dtype=F64):
    """reorder_first_stage_pred_and_feature -> rois (B, M, cols), roi_scores, roi_labels (int64), roi_features"""
    B, cols = len(pred), np.shape(pred[0]["box3d_lidar"])[1]
    rois, scores = torch.zeros((B, M, cols), dtype=dtype), torch.zeros((B, M), dtype=dtype)
    labels, features = torch.zeros((B, M), dtype=torch.long), torch.zeros((B, M, feats[0].shape[1]), dtype=dtype)
    for i in range(B):
        n = feats[i].shape[0]
        box = _t(pred[i]["box3d_lidar"], dtype)
        if code_size == 9:
            box = box[:, [0, 1, 2, 3, 4, 5, 8, 6, 7]]
        rois[i, :n], scores[i, :n], features[i, :n] = box, _t(pred[i]["scores"], dtype), feats[i]
        labels[i, :n] = torch.as_tensor(np.asarray(pred[i]["label_preds"])) + 1
    return rois, scores, labels, features


def mlp(sd, cfg, feats, dtype=F64, fault=None):
    """shared_fc_layer, cls_layers, reg_layers in eval mode from the unfolded parameters: feats (N, c_in) -> cls (N, 1),
    reg (N, code_size)"""
    eps = 1e-3 if fault == "eps_1e-3" else 1e-5
    x = _t(feats, dtype).unsqueeze(-1)
    outs, shared = {}, None
    for conv, bn, _ in layer_names(cfg):
        if conv.endswith(".0.") and not conv.startswith("shared"):
            if shared is None:
                shared = x
            x = shared
        bias = sd.get(conv + "bias")
        x = F.conv1d(x, _t(sd[conv + "weight"], dtype), None if bias is None else _t(bias, dtype))
        if bn is not None:
            g, beta, mean, var = (_t(v, dtype) for v in bn_of(sd, bn))
            x = F.relu(F.batch_norm(x, mean, var, g, beta, False, 0.0, eps))
        else:
            outs[conv.split("_")[0]] = x.squeeze(-1)
    return outs["cls"], outs["reg"]


def predicted_boxes(rois, reg, fault=None):
    """generate_predicted_boxes: rois (B, M, code) with the rotation at column 6, reg (B * M, code) -> (B, M, code)"""
    B, M, code = rois.shape
    ry, xyz = rois[:, :, 6].reshape(-1), rois[:, :, 0:3].reshape(-1, 3)
    local = rois.clone()
    local[:, :, 0:3] = 0
    pred = (reg.view(B, M, code) + local).view(-1, code)
    c, s = torch.cos(ry), torch.sin(ry)
    zeros, ones = torch.zeros_like(ry), torch.ones_like(ry)
    rot = torch.stack((c, -s, zeros, s, c, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3)
    head = torch.matmul(pred[:, None, 0:3], rot)[:, 0]
    pred = torch.cat((head, pred[:, 3:]), -1)
    if fault == "velocity_rotated" and code == 9:
        vel = torch.cat((pred[:, 7:9], zeros[:, None]), -1)
        pred = torch.cat((pred[:, :7], torch.matmul(vel[:, None], rot)[:, 0, :2]), -1)
    pred = torch.cat((pred[:, 0:3] + xyz, pred[:, 3:]), -1)
    return pred.view(B, M, code)


def post_process(box_preds, cls_preds, roi_scores, roi_labels, fault=None):
    """post_process -> per sample (boxes, scores, labels int64)"""
    out = []
    for i in range(box_preds.shape[0]):
        box = box_preds[i]
        if box.shape[-1] == 9:
            box = box[:, [0, 1, 2, 3, 4, 5, 7, 8, 6]]
        score = torch.sigmoid(cls_preds[i]).reshape(-1) * roi_scores[i].reshape(-1)
        if fault != "sqrt_dropped":
            score = torch.sqrt(score)
        mask = (roi_labels[i] != 0).reshape(-1)
        out.append((box[mask], score[mask], roi_labels[i][mask] - (0 if fault == "labels_not_shifted" else 1)))
    return out


def second_stage(sd, cfg, code_size, bev, pred, M=GOLDEN_M, num_point=NUM_POINT, ext=EXTRACTOR, dtype=F64, fault=None):
    """everything after the first stage -> a dict of every intermediate: centres, features, rois, roi_scores, roi_labels,
    roi_features, cls, box_preds, final (post_process's list)"""
    centres = [box_points(p["box3d_lidar"], num_point, dtype, fault) for p in pred]
    feats = bev_features(bev, centres, num_point, ext, dtype, fault)
    rois, scores, labels, features = reorder(pred, feats, M, code_size, dtype)
    cls, reg = mlp(sd, cfg, features.view(-1, features.shape[-1]), dtype, fault)
    box = predicted_boxes(rois, reg, fault)
    cls = cls.view(rois.shape[0], M, 1)
    return dict(centres=centres, features=feats, rois=rois, roi_scores=scores, roi_labels=labels, roi_features=features, cls=cls,
                box_preds=box, final=post_process(box, cls, scores, labels, fault))


def golden_case(code_size):
    """the seeded inputs of golden case c7 / c9: weights, config, map, first-stage list"""
    tag = f"c{code_size}"
    return dict(sd=head_weights(NUM_POINT * MAP["C"], SMALL, code_size, tag), cfg=SMALL, bev=bev_map(), pred=first_pred(tag, code_size))


PROD_ROWS = 37


def production_case():
    """RoIHead alone at the production widths: 37 RoIs of 2560 features"""
    feats = np.maximum(synth.uniform(SEED, "prod/f", (1, PROD_ROWS, 2560), -0.5, 2.0), 0.0).astype(np.float32)
    rois = boxes("prod/rois", PROD_ROWS, 9)[:, [0, 1, 2, 3, 4, 5, 8, 6, 7]][None]
    scores = synth.uniform(SEED, "prod/s", (1, PROD_ROWS), 0.1, 0.95).astype(np.float32)
    return dict(sd=head_weights(2560, PRODUCTION, 9, "prod"), cfg=PRODUCTION, rois=rois, roi_scores=scores, roi_features=feats)


def head_alone(case, dtype=F64, fault=None):
    """RoIHead.forward on given rois / features -> (cls (B, M, 1), box_preds (B, M, code))"""
    rois, feats = _t(case["rois"], dtype), _t(case["roi_features"], dtype)
    cls, reg = mlp(case["sd"], case["cfg"], feats.view(-1, feats.shape[-1]), dtype, fault)
    return cls.view(rois.shape[0], rois.shape[1], 1), predicted_boxes(rois, reg, fault)
