#!/usr/bin/env python3
"""Generate tests/golden/live_reference.npz: the REAL reference's (jacky121298/3DAL_PyTorch) outputs on the extra
cases of tests/test_oracle_live_reference.py — other seeds, ragged N, an all-background crop, more geometry seeds and
the loss modules on another seed. Run only where a reference checkout exists:
    DAL3_REFERENCE=<checkout> python tests/golden/gen_live_reference.py

The reference is imported (never copied) through the shim of gen_golden.py. Stored per case: the segmentation-bias
shift the reference's own logits gave (`*_margin`; the test re-centres synth's weights with it) and the reference's
OUTPUTS. The inputs are rebuilt from 3dal_pytorch_amd/synth.py wherever the fixture is used; `*_in_sum` guards them.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
synth = importlib.import_module("3dal_pytorch_amd.synth")
import gen_golden as G                                        # noqa: E402  (the import shim lives there)

STATIC_ONE = [(700, 3), (1024, 4), (96, 5)]
GEOM = [(51, np.float32), (52, np.float64), (53, np.float32)]


def main():
    torch.set_grad_enabled(False)
    sm, dm, se, de, ut = G.import_reference()
    out = {}

    def put(prefix, d):
        d = G.tonp(d)
        out[f"{prefix}_keys"] = np.array(list(d.keys()))
        for k, v in d.items():
            out[f"{prefix}_{k}"] = v

    for n, seed in STATIC_ONE:
        pts_np, init_np, gt_np = synth.static_crops(3, n, seed=seed)
        pts_np[2] *= 100.0
        pts = torch.from_numpy(pts_np).transpose(2, 1)
        model = sm.StaticModelOneBoxEst(3, 3)
        _, mm = G.centred_sd("static_one", model, pts, seed)
        np.random.seed(99)
        put(f"static_one_{n}_{seed}", model(pts, torch.from_numpy(init_np), torch.from_numpy(gt_np)))
        out[f"static_one_{n}_{seed}_margin"] = np.float64(mm)
        out[f"static_one_{n}_{seed}_in_sum"] = np.float64(pts_np.astype(np.float64).sum() + init_np.astype(np.float64).sum())

    pts_np, init_np, gt_np = synth.static_crops(3, 640, seed=8)
    pts = torch.from_numpy(pts_np).transpose(2, 1)
    model = sm.StaticModelTwoBoxEst(3, 3)
    _, mm = G.centred_sd("static_two", model, pts, 8)
    np.random.seed(5)
    put("static_two", model(pts, torch.from_numpy(init_np), torch.from_numpy(gt_np)))
    out["static_two_margin"] = np.float64(mm)
    out["static_two_in_sum"] = np.float64(pts_np.astype(np.float64).sum() + init_np.astype(np.float64).sum())

    pts_np, box_np, init8_np, gt_np = synth.dynamic_items(2, n_per_frame=256, seed=21)
    pts = torch.from_numpy(pts_np).transpose(2, 1)
    box = torch.from_numpy(box_np).transpose(2, 1)
    model = dm.DynamicModel(3, 4)
    _, mm = G.centred_sd("dynamic", model, pts, 21)
    np.random.seed(6)
    put("dynamic", model(pts, box, torch.from_numpy(gt_np)))
    out["dynamic_margin"] = np.float64(mm)
    out["dynamic_in_sum"] = np.float64(pts_np.astype(np.float64).sum() + box_np.astype(np.float64).sum())

    geo, ops, wc = G.import_reference_geometry()
    for seed, dt in GEOM:
        pts, box9, _, _, _ = synth.sweep(seed, "live", n_points=3000, n_boxes=7)
        boxes = np.concatenate([box9[:, :3], box9[:, [4, 3, 5]], (-box9[:, -1:] - np.pi / 2)], 1).astype(dt)
        pts = pts.astype(dt)
        out[f"geom_{seed}_in_rbbox"] = ops.points_in_rbbox(pts, boxes)
        nv, d = geo.surface_equ_3d_jitv2(ops.corner_to_surfaces_3d(
            ops.center_to_corner_box3d(boxes[:, :3], boxes[:, 3:6], boxes[:, -1]))[:, :, :3, :])
        out[f"geom_{seed}_normal"], out[f"geom_{seed}_d"] = nv, d
        out[f"geom_{seed}_in_sum"] = np.float64(pts.astype(np.float64).sum() + boxes.astype(np.float64).sum())

    torch.set_grad_enabled(True)
    for name, crit, two in (("one", sm.FrustumPointNetLossOneBoxEst(), False),
                            ("two", sm.FrustumPointNetLossTwoBoxEst(), True),
                            ("dynamic", dm.DynamicModelLoss(), False)):
        out_np, labels_np = synth.loss_case(77, two_stage=two, batch=5, n_pts=40)
        out_t = {k: torch.from_numpy(v).requires_grad_(v.dtype == np.float32) for k, v in out_np.items()}
        lo = crit(out_t, *[torch.from_numpy(a) for a in labels_np], w_box=0.7)
        g, = torch.autograd.grad(lo["total_loss"], [out_t["logits"]])
        out[f"loss_{name}_keys"] = np.array(list(lo.keys()))
        out[f"loss_{name}_values"] = np.array([float(v.detach()) for v in lo.values()], dtype=np.float64)
        out[f"loss_{name}_grad_logits"] = g.numpy()

    path = os.path.join(HERE, "live_reference.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
