#!/usr/bin/env python3
"""Generate tests/golden/roi.npz from the REAL reference (jacky121298/3DAL_PyTorch): its own `RoIHead`
(det3d/models/roi_heads/roi_head.py, roi_head_template.py), `BEVFeatureExtractor` (det3d/models/second_stage/bird_eye_view.py
with det3d/core/utils/center_utils.py's bilinear_interpolate_torch) and `TwoStageDetector.get_box_center`,
`reorder_first_stage_pred_and_feature` and `post_process` (det3d/models/detectors/two_stage.py with
det3d/core/bbox/box_torch_ops.py), on the seeded inputs and weights of tests/roi_ref.py.

Run only where the reference checkout exists (DAL3_REFERENCE, as tests/golden/gen_pillars.py reads it):
    python tests/golden/gen_roi.py

The files are loaded by path behind stub modules for what their import chain needs and this machine lacks: the
registries, BaseDetector (nn.Module), the builder, ProposalTargetLayer (a parameter-free nn.Module that keeps its
configuration), the iou3d CUDA extension and circle_nms. box_torch_ops.torch_to_np_dtype has no float64 entry; the .double()
run gives it one, and keeps rotate_points_along_z's matrix in float64 (its `.float()` would make torch.matmul refuse the
operands: Tensor.float is the identity on float64 tensors while that run lasts). The detector's three methods are called unbound on a stand-in `self` that carries num_point,
NMS_POST_MAXSIZE and the real RoIHead.

What is recorded, for code sizes 7 and 9 (cases c7, c9; 5 points, a 2 x 6 x 9 x 20 map, 40 and 23 boxes in 48 slots, the
[32, 32] / [16, 48] head): the box points, the point features, RoIHead's batch_cls_preds and batch_box_preds, and
post_process's boxes, scores and labels, each from the fp32 modules and from the same modules' .double() copies on the
same inputs (the truth, stored as the fp32 output plus a float32 difference); RoIHead alone at the production widths on 37
RoIs (case prod); RoIHead's key list with shapes. tests/roi_ref.py's restatement is asserted here against both runs.
Fixed timestamps: a rerun reproduces the archive byte for byte.
"""
import copy
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gen_pillars as G  # noqa: E402
import roi_ref as R  # noqa: E402


class Cfg(dict):
    """a config dict read by attribute, as the reference's config loader hands it over"""

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        v = self[k]
        return Cfg(v) if isinstance(v, dict) else v


def import_reference():
    G.import_reference()

    class Registry:
        @staticmethod
        def register_module(cls):
            return cls

    class ProposalTargetLayer(nn.Module):
        def __init__(self, roi_sampler_cfg):
            super().__init__()
            self.roi_sampler_cfg = roi_sampler_cfg

    for name in ["det3d.ops.iou3d_nms", "det3d.core.bbox", "det3d.core.utils", "det3d.models.detectors", "det3d.models.roi_heads",
                 "det3d.models.roi_heads.target_assigner", "det3d.models.second_stage", "det3d.models.builder"]:
        G._stub(name)
    sys.modules["det3d.ops.iou3d_nms"].__dict__.update(iou3d_nms_cuda=None, iou3d_nms_utils=None)
    G._stub("det3d.core.utils.circle_nms_jit", circle_nms=None)
    G._stub("det3d.models.detectors.base", BaseDetector=nn.Module)
    G._stub("det3d.models.roi_heads.target_assigner.proposal_target_layer", ProposalTargetLayer=ProposalTargetLayer)
    sys.modules["det3d.models"].builder = sys.modules["det3d.models.builder"]
    sys.modules["det3d.models.registry"].__dict__.update(DETECTORS=Registry, ROI_HEAD=Registry, SECOND_STAGE=Registry)
    ops = G._load_file("det3d.core.bbox.box_torch_ops", "det3d/core/bbox/box_torch_ops.py")
    to_np = ops.torch_to_np_dtype
    ops.torch_to_np_dtype = lambda t: np.dtype(np.float64) if t == torch.float64 else to_np(t)
    sys.modules["det3d.core.bbox"].box_torch_ops = ops
    sys.modules["det3d.core"].box_torch_ops = ops
    G._load_file("det3d.core.utils.center_utils", "det3d/core/utils/center_utils.py")
    G._load_file("det3d.models.roi_heads.roi_head_template", "det3d/models/roi_heads/roi_head_template.py")
    head = G._load_file("det3d.models.roi_heads.roi_head", "det3d/models/roi_heads/roi_head.py")
    bev = G._load_file("det3d.models.second_stage.bird_eye_view", "det3d/models/second_stage/bird_eye_view.py")
    two = G._load_file("det3d.models.detectors.two_stage", "det3d/models/detectors/two_stage.py")
    return head, bev, two


class keep_double:
    """while it lasts, Tensor.float() leaves a float64 tensor as it is"""

    def __enter__(self):
        self.orig = orig = torch.Tensor.float
        torch.Tensor.float = lambda t, *a, **k: t if t.dtype == torch.float64 else orig(t, *a, **k)

    def __exit__(self, *exc):
        torch.Tensor.float = self.orig


def build_head(mod, input_channels, cfg, code_size, sd):
    head = mod.RoIHead(input_channels, Cfg(cfg), num_class=1, code_size=code_size)
    head.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    return head.eval()


def run_reference(head, ext, two, bev, pred, dtype):
    """the reference's forward after the first stage, at `dtype` -> roi_ref.second_stage's dict"""
    head = copy.deepcopy(head).to(dtype)
    me = types.SimpleNamespace(num_point=R.NUM_POINT, NMS_POST_MAXSIZE=R.GOLDEN_M, roi_head=head)
    first = [{"box3d_lidar": torch.from_numpy(p["box3d_lidar"]).to(dtype), "scores": torch.from_numpy(p["scores"]).to(dtype),
              "label_preds": torch.from_numpy(p["label_preds"])} for p in pred]
    example = {"bev_feature": torch.from_numpy(bev).to(dtype), "metadata": [None] * len(pred)}
    T = two.TwoStageDetector
    centres = T.get_box_center(me, first)
    feats = ext.forward(example, centres, R.NUM_POINT)
    example = T.reorder_first_stage_pred_and_feature(me, first_pred=first, example=example, features=[feats])
    with keep_double():
        out = head(example, training=False)
    final = T.post_process(me, out)
    return dict(centres=centres, features=feats, cls=out["batch_cls_preds"], box_preds=out["batch_box_preds"],
                final=[(d["box3d_lidar"], d["scores"], d["label_preds"]) for d in final])


def flat(r):
    """the recorded arrays of a run"""
    return {"centres": torch.cat(r["centres"]).numpy(), "features": torch.cat(r["features"]).numpy(), "cls": r["cls"].numpy(),
            "box_preds": r["box_preds"].numpy(), "final_boxes": torch.cat([f[0] for f in r["final"]]).numpy(),
            "final_scores": torch.cat([f[1] for f in r["final"]]).numpy()}


def store(out, tag, name, f32, f64):
    f32 = np.asarray(f32, np.float32)
    out[f"{tag}_{name}_f32"], out[f"{tag}_{name}_diff"] = f32, (f64 - f32.astype(np.float64)).astype(np.float32)
    back = f32.astype(np.float64) + out[f"{tag}_{name}_diff"].astype(np.float64)
    assert np.abs(back - f64).max() <= 1e-12 * max(np.abs(f64).max(), 1.0), (tag, name)


def main():
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    hmod, bmod, two = import_reference()
    ext = bmod.BEVFeatureExtractor(**R.EXTRACTOR)
    out = {}
    for code in (7, 9):
        tag, case = f"c{code}", R.golden_case(code)
        head = build_head(hmod, R.NUM_POINT * R.MAP["C"], case["cfg"], code, case["sd"])
        assert head.shared_fc_layer[1].eps == 1e-5
        runs = {dt: run_reference(head, ext, two, case["bev"], case["pred"], dt) for dt in (torch.float32, torch.float64)}
        mine = {dt: R.second_stage(case["sd"], case["cfg"], code, case["bev"], case["pred"], dtype=dt) for dt in runs}
        a32, a64, m32, m64 = flat(runs[torch.float32]), flat(runs[torch.float64]), flat(mine[torch.float32]), flat(mine[torch.float64])
        for name in a64:
            err = np.abs(m64[name] - a64[name]).max() / max(np.abs(a64[name]).max(), 1e-30)
            assert err < 1e-11, (tag, name, err)
            same = np.array_equal(m32[name], a32[name])
            print(f"{tag} {name:13s} {a64[name].shape}: restatement f64 err {err:.1e}, f32 bits {'equal' if same else 'differ'}; fp32 own "
                  f"error {R.judge(a32[name].reshape(-1, a32[name].shape[-1]) if a32[name].ndim > 1 else a32[name][:, None], a64[name].reshape(-1, a64[name].shape[-1]) if a64[name].ndim > 1 else a64[name][:, None])}")
            assert same or name in ("cls", "box_preds", "final_boxes", "final_scores"), (tag, name)
            store(out, tag, name, a32[name], a64[name])
        labels = torch.cat([f[2] for f in runs[torch.float32]["final"]]).numpy()
        assert np.array_equal(labels, torch.cat([f[2] for f in mine[torch.float64]["final"]]).numpy())
        out[f"{tag}_final_labels"] = labels.astype(np.int64)
        out[f"{tag}_final_counts"] = np.asarray([f[0].shape[0] for f in runs[torch.float32]["final"]], np.int64)
        assert tuple(out[f"{tag}_final_counts"]) == R.GOLDEN_BOXES
    # ---- RoIHead alone at the production widths
    case = R.production_case()
    head = build_head(hmod, 2560, case["cfg"], 9, case["sd"])
    res = {}
    for dt in (torch.float32, torch.float64):
        h = copy.deepcopy(head).to(dt)
        with keep_double():
            d = h({k: torch.from_numpy(case[k]).to(dt) for k in ("rois", "roi_scores", "roi_features")}, training=False)
        res[dt] = (d["batch_cls_preds"].numpy(), d["batch_box_preds"].numpy())
    mine = R.head_alone(case)
    for i, name in enumerate(("cls", "box_preds")):
        err = np.abs(mine[i].numpy() - res[torch.float64][i]).max() / np.abs(res[torch.float64][i]).max()
        assert err < 1e-11, ("prod", name, err)
        store(out, "prod", name, res[torch.float32][i], res[torch.float64][i])
        print(f"prod {name}: rms {np.sqrt((res[torch.float64][i] ** 2).mean()):.3f}, restatement f64 err {err:.1e}")
    keys, shapes = [], []
    for k, v in head.state_dict().items():
        keys.append(k)
        shapes.append(list(v.shape) + [0] * (3 - v.dim()))
    out["keys"] = np.asarray(keys)
    out["key_shapes"] = np.asarray(shapes, np.int64)
    path = os.path.join(HERE, "roi.npz")
    G.save(path, out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
