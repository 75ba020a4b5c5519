#!/usr/bin/env python3
"""Generate tests/golden/center_loss.npz from the REAL reference (jacky121298/3DAL_PyTorch): its own `AssignLabel.__call__`
(det3d/datasets/pipelines/preprocess.py, train mode, the Waymo and the nuScenes branch), `FastFocalLoss` and `RegLoss`
(det3d/models/losses/centernet_loss.py) and `CenterHead.loss` (det3d/models/bbox_heads/center_head.py), on the seeded inputs of
tests/center_ref.py.

Run only where the reference checkout exists (DAL3_REFERENCE, as tests/golden/gen_pillars.py reads it):
    python tests/golden/gen_center_loss.py

The files are loaded by path behind gen_rpn.py's stubs. What this machine lacks is replaced, nothing else: numba's
decorators (identity), the database sampler's builder and the pipeline registry (never called here). The assigner gets what
the pipeline would hand it: the per-sample annotations cut from the collated rows (x, y, z, w, l, h, vx, vy, rot, the class
apart), and `voxels` with the float32 `range` and `size` and the int64 `shape` of the reference's VoxelGenerator, which is
asked for them.

What is recorded, for the inputs `main` and `empty` (a task without any object): the targets of every task (hm, anno_box,
ind, mask, cat, stacked over the two samples; anno_box also as a float32 difference to the float64 value of its log / sin /
cos columns), and for the code sizes c10 (nuScenes weights, with vel) and c8 (Waymo weights, without) CenterHead.loss's four
outputs and autograd's gradients of `loss` in every head map, each from the fp32 call and from .double() copies of the same
inputs (stored as the fp32 output plus a float32 difference). tests/center_ref.py's restatement is asserted against all of
it, and so are the conditions under which rounding cannot move a discrete decision. Fixed timestamps: a rerun reproduces the
archive byte for byte."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gen_pillars as G  # noqa: E402
import gen_roi as GR  # noqa: E402
import gen_rpn as GN  # noqa: E402
import center_ref as T  # noqa: E402

LOSS_KEYS = ("loss", "hm_loss", "loc_loss", "loc_loss_elem", "num_positive")


class Cfg(dict):
    __getattr__ = dict.__getitem__


def import_reference():
    GN.import_reference()
    sys.modules["numba"].njit = sys.modules["numba"].jit

    class Registry:
        @staticmethod
        def register_module(cls):
            return cls

    for name in ["det3d.core.bbox", "det3d.core.sampler", "det3d.datasets", "det3d.datasets.pipelines"]:
        G._stub(name)
    G._stub("det3d.builder", build_dbsampler=None)
    G._stub("det3d.datasets.registry", PIPELINES=Registry)
    G._load_file("det3d.core.bbox.geometry", "det3d/core/bbox/geometry.py")
    ops = G._load_file("det3d.core.bbox.box_np_ops", "det3d/core/bbox/box_np_ops.py")
    sys.modules["det3d.core.bbox"].box_np_ops = ops
    G._stub("det3d.core.sampler.preprocess")
    sys.modules["det3d.core.sampler"].preprocess = sys.modules["det3d.core.sampler.preprocess"]
    G._load_file("det3d.core.utils.center_utils", "det3d/core/utils/center_utils.py")
    G._load_file("det3d.models.losses.centernet_loss", "det3d/models/losses/centernet_loss.py")
    head = G._load_file("det3d.models.bbox_heads.center_head", "det3d/models/bbox_heads/center_head.py")
    pre = G._load_file("det3d.datasets.pipelines.preprocess", "det3d/datasets/pipelines/preprocess.py")
    gen = sys.modules["det3d.core.input.voxel_generator"]
    return pre, head, gen


def reference_targets(pre, gen, gt, kind):
    """AssignLabel.__call__ per sample -> center_ref.targets' dictionary (stacked over the samples)"""
    vg = gen.VoxelGenerator(voxel_size=[0.1, 0.1, 0.15], point_cloud_range=[-9.6, -8.0, -3.0, 9.6, 8.0, 3.0], max_num_points=5)
    voxels = dict(shape=vg.grid_size, range=vg.point_cloud_range, size=vg.voxel_size)
    for k in ("shape", "range", "size"):
        assert voxels[k].dtype == T.VOXELS[k].dtype and np.array_equal(voxels[k], T.VOXELS[k]), k
    cfg = Cfg(T.ASSIGNER, target_assigner=Cfg(tasks=[Cfg(t) for t in T.TASKS]))
    assigner = pre.AssignLabel(cfg=cfg)
    names = np.array([n for t in T.TASKS for n in t["class_names"]])
    per = []
    for b in range(gt.shape[0]):
        rows = gt[b][gt[b, :, 9] != 0]
        ann = dict(gt_boxes=rows[:, [0, 1, 2, 3, 4, 5, 7, 8, 6]].copy(), gt_classes=rows[:, 9].astype(np.int32),
                   gt_names=names[rows[:, 9].astype(np.int64) - 1])
        res = dict(mode="train", type=kind, lidar=dict(voxels=voxels, annotations=ann))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)         # the NaN and the 1e20 row's casts
            res, _ = assigner(res, None)
        ex = res["lidar"]["targets"]
        # the collated tensor is these rows without the gaps: the order the kernel relies on
        assert np.array_equal(ex["gt_boxes_and_cls"][:len(rows)], rows, equal_nan=True) and not ex["gt_boxes_and_cls"][len(rows):].any()
        per.append(ex)
    return {k: [np.stack([ex[k][t] for ex in per]) for t in range(len(T.TASKS))] for k in ("hm", "anno_box", "ind", "mask", "cat")}


def reference_loss(hmod, code, preds, tg, dtype):
    """CenterHead.loss on leaves' copies (the reference's sigmoid_ is in place) -> center_ref.loss's list"""
    dataset, cw, weight, with_vel = T.CODES[code]
    common = dict(T.HEADS9 if with_vel else T.HEADS7)
    head = hmod.CenterHead(in_channels=16, tasks=T.TASKS, dataset=dataset, weight=weight, code_weights=cw, common_heads=common,
                           share_conv_channel=64)
    leaves = [{h: T._t(v, dtype).clone().requires_grad_(True) for h, v in p.items()} for p in preds]
    example = {k: [T._t(v, dtype) for v in tg[k]] for k in ("hm", "anno_box", "ind", "mask", "cat")}
    rets = head.loss(example, [{h: v * 1 for h, v in p.items()} for p in leaves])
    sum(rets["loss"]).backward()
    out = []
    for t, p in enumerate(leaves):
        r = {k: rets[k][t].detach().numpy() for k in LOSS_KEYS}
        r.update({f"grad.{h}": v.grad.numpy() for h, v in p.items()})
        out.append(r)
    return out


def check_stability(tag, gt, detail):
    """rounding cannot move a discrete decision: no radius within 1e-4 relative of an integer, no centre coordinate within
    1e-4 of a cell boundary; the nearly-in-range centre sits well inside (-1, 0)"""
    near = 0
    for b, t, k, rad, fx, fy in detail:
        assert abs(rad - round(rad)) > 1e-4 * rad, (tag, b, t, k, rad)
        for v in (fx, fy):
            if np.isfinite(v) and abs(v) < 1e6:
                assert abs(v - round(float(v))) > 1e-4, (tag, b, t, k, v)
                if -1 < v < 0:
                    assert -0.9 < v < -0.1, (tag, v)
                    near += 1
    assert near >= 1, tag


def main():
    torch.set_num_threads(1)
    pre, hmod, gen = import_reference()
    out = {}
    for tag in ("main", "empty"):
        gt = T.golden_gt(tag)
        ref = reference_targets(pre, gen, gt, "WaymoDataset")
        nus = reference_targets(pre, gen, gt, "NuScenesDataset")
        detail = []
        mine = T.targets(gt, T.NUM_CLASSES, T.VOXELS, 8, (T.H, T.W), detail=detail)
        check_stability(tag, gt, detail)
        for t in range(len(T.TASKS)):
            for k in ("hm", "anno_box", "ind", "mask", "cat"):
                a = ref[k][t]
                assert a.dtype == mine[k][t].dtype and np.array_equal(a, nus[k][t]) and np.array_equal(a, mine[k][t]), (tag, t, k)
                if k not in ("hm", "anno_box"):
                    out[f"{tag}_t{t}_{k}"] = a
            out[f"{tag}_t{t}_hm"] = ref["hm"][t]
            GR.store(out, f"{tag}_t{t}", "anno_box", ref["anno_box"][t], mine["anno_box64"][t])
            print(f"{tag} task {t}: {int(ref['mask'][t].sum())} live slots, hm max {ref['hm'][t].max():g}, "
                  f"{int((ref['hm'][t] > 0).sum())} lit pixels")
        for code, (_, cw, weight, with_vel) in T.CODES.items():
            preds = T.head_maps(f"{tag}/{code}", ref, T.NUM_CLASSES, with_vel)
            r32, r64 = (reference_loss(hmod, code, preds, ref, dt) for dt in (T.F32, T.F64))
            m32, m64 = (T.loss(preds, ref, cw, weight, dt) for dt in (T.F32, T.F64))
            for t in range(len(T.TASKS)):
                for name in r64[t]:
                    a32, a64 = np.asarray(r32[t][name]), np.asarray(r64[t][name])
                    err = np.abs(m64[t][name] - a64).max() / max(np.abs(a64).max(), 1e-30)
                    same = np.array_equal(m32[t][name], a32)
                    print(f"{tag} {code} task {t} {name:14s} {str(a64.shape):16s} restatement f64 err {err:.1e}, f32 bits {'equal' if same else 'differ'}")
                    assert err < 1e-12 and same, (tag, code, t, name, err)
                    GR.store(out, f"{tag}_{code}_t{t}", name, a32, a64)
                g = r32[t]["grad.hm"]
                p = 1 / (1 + np.exp(-np.float64(preds[t]["hm"])))
                assert (g[(p < 9e-5) | (p > 1 - 9e-5)] == 0).all() and ((p < 9e-5) | (p > 1 - 9e-5)).sum() >= 4
    path = os.path.join(HERE, "center_loss.npz")
    G.save(path, out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
