#!/usr/bin/env python3
"""Generate tests/golden/nms.npz from the REAL reference (jacky121298/3DAL_PyTorch): its own `rotate_nms_pcdet`
(det3d/core/bbox/box_torch_ops.py:248), `circle_nms` (det3d/core/utils/circle_nms_jit.py) behind `_circle_nms`, and
`CenterHead.predict` / `post_processing` (det3d/models/bbox_heads/center_head.py:294-506), on the seeded inputs of
tests/nms_ref.py (clustered_scene, head_maps; rebuilt from their seeds where the fixture is used).

Run only where the reference checkout exists (DAL3_REFERENCE, default /root/reference):
    python tests/golden/gen_nms.py

center_head.py, box_torch_ops.py and circle_nms_jit.py are loaded by path with stub modules for what their import chain
needs and this machine lacks (numba with `jit` as identity, the det3d packages around them, the CUDA extension).
The one substitution: `iou3d_nms_cuda.nms_gpu` is CUDA-only, so it is replaced by a recorder that runs the greedy scan
over the reference's own CPU IoU (`boxes_iou_bev_cpu`, compiled out of tree as gen_iou_golden.py does) on the
pcdet-mirrored boxes it is handed; `Tensor.cuda` is the identity while the reference runs.

The margins are conditions: seeds are searched until no pair's IoU lies within 1e-4 of the threshold (for the
reference's CPU IoU AND tests/iou_ref.py's float64 IoU, both on the same side), no squared centre distance within 1e-4
of a radius, no two scores of a segment are equal, no sigmoid score within 1e-5 of the score threshold and no centre
within 1e-3 m of a face of the range. They are asserted.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gen_iou_golden  # noqa: E402  (reference_iou_bev_cpu)
import iou_ref  # noqa: E402
import nms_ref  # noqa: E402

REF = gen_iou_golden.REF
RECORD = []                                     # one entry per nms_gpu call: the IoU matrix it scanned


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    mod.__path__ = []
    mod.__dict__.update(attrs)
    sys.modules[name] = mod
    return mod


def _load_file(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_reference(iou_cpu):
    def nms_gpu(boxes, keep, thresh):
        n = boxes.shape[0]
        iou = torch.zeros((n, n), dtype=torch.float32)
        iou_cpu(boxes.contiguous(), boxes.contiguous(), iou)
        kept = nms_ref.greedy(iou.numpy() > np.float32(thresh))
        keep[:kept.size] = torch.from_numpy(kept)
        RECORD.append(iou.numpy().copy())
        return int(kept.size)

    def jit(*args, **kwargs):
        return args[0] if args and callable(args[0]) else (lambda fn: fn)

    class Registry:
        @staticmethod
        def register_module(cls):
            return cls

    _stub("numba", jit=jit)
    for name in ["det3d", "det3d.core", "det3d.core.bbox", "det3d.core.utils", "det3d.ops", "det3d.torchie", "det3d.models",
                 "det3d.models.losses", "det3d.models.bbox_heads", "torchvision", "spconv"]:
        if name not in sys.modules or name.startswith("det3d"):
            _stub(name)
    cuda = _stub("det3d.ops.iou3d_nms.iou3d_nms_cuda", nms_gpu=nms_gpu)
    _stub("det3d.ops.iou3d_nms", iou3d_nms_cuda=cuda, iou3d_nms_utils=None)
    _stub("det3d.torchie.cnn", kaiming_init=None)
    _stub("det3d.models.losses.centernet_loss", FastFocalLoss=None, RegLoss=None)
    _stub("det3d.models.utils", Sequential=torch.nn.Sequential)
    _stub("det3d.models.registry", HEADS=Registry)
    ops = _load_file("det3d.core.bbox.box_torch_ops", "det3d/core/bbox/box_torch_ops.py")
    sys.modules["det3d.core"].box_torch_ops = ops
    _load_file("det3d.core.utils.circle_nms_jit", "det3d/core/utils/circle_nms_jit.py")
    head = _load_file("det3d.models.bbox_heads.center_head", "det3d/models/bbox_heads/center_head.py")
    return ops, head


def rotate_margin_ok(boxes7, order, thresh, iou_cpu_matrix):
    """no pair of the candidates within 1e-4 of thresh, for both IoUs, on the same side"""
    m = order.size
    assert iou_cpu_matrix.shape == (m, m)
    iu = np.triu_indices(m, 1)
    a = iou_cpu_matrix.astype(np.float64)[iu]
    conv = nms_ref.mirrored(boxes7[order])      # the float32 boxes the reference hands to nms_gpu
    b = iou_ref.pairwise(conv, conv)[0][iu]
    return bool(np.all(np.abs(a - thresh) > 1e-4) and np.all(np.abs(b - thresh) > 1e-4) and np.all((a > thresh) == (b > thresh)))


def circle_margin_ok(xy, thresh):
    d = xy[:, None, :].astype(np.float64) - xy[None, :, :].astype(np.float64)
    d2 = (d ** 2).sum(-1)[np.triu_indices(xy.shape[0], 1)]
    return bool(np.all(np.abs(d2 - thresh) > 1e-4))


def scene(ops, head):
    for seed in range(200):
        boxes, scores = nms_ref.clustered_scene(seed)
        if np.unique(scores).size != scores.size:
            continue
        out, ok = {}, True
        for name, (mode, thresh, pre, post) in nms_ref.SCENE_CASES.items():
            if mode == "rotate":
                RECORD.clear()
                keep = ops.rotate_nms_pcdet(torch.from_numpy(boxes.copy()), torch.from_numpy(scores.copy()), thresh=thresh,
                                            pre_maxsize=pre, post_max_size=post).numpy()
                ok = ok and rotate_margin_ok(boxes, nms_ref.order(scores)[:pre], thresh, RECORD[-1])
            else:
                dets = torch.from_numpy(np.concatenate([boxes[:, :2], scores[:, None]], 1))
                keep = head._circle_nms(dets, min_radius=thresh, post_max_size=post).numpy()
                ok = ok and circle_margin_ok(boxes[:, :2], thresh)
            out[f"scene_{name}_keep"] = keep.astype(np.int64)
        if not ok:
            continue
        # how much the sequential dependence matters in this scene
        o = nms_ref.order(scores)
        sup = nms_ref.suppression(nms_ref.mirrored(boxes[o]), "rotate", 0.7)
        any_higher = int((~np.triu(sup, 1).any(0)).sum())
        print(f"scene: seed {seed}, {boxes.shape[0]} boxes, {int(np.triu(sup, 1).sum())} overlapping pairs, greedy keeps "
              f"{nms_ref.greedy(sup).size}, 'no higher box overlaps' keeps {any_higher}")
        for name, (mode, thresh, pre, post) in nms_ref.SCENE_CASES.items():
            mine = nms_ref.nms(boxes, scores, mode, thresh, pre, post, mirror=True)
            assert np.array_equal(mine, out[f"scene_{name}_keep"]), name
            print(f"  {name}: keeps {mine.size}")
        out.update(scene_seed=seed, scene_sum=float(boxes.astype(np.float64).sum() + scores.astype(np.float64).sum()))
        return out
    raise RuntimeError("no scene seed satisfies the margins")


HEAD_RUNS = {"ref_vel": ("ref", True), "ref_novel": ("ref", False), "small_vel": ("small", True), "circle_vel": ("circle", True)}


def head_run(head, seed, cfg_name, vel):
    """-> (arrays, ok)"""
    cfg = nms_ref.CONFIGS[cfg_name]
    tasks = nms_ref.head_maps(seed, vel)
    captured = []
    fake = types.SimpleNamespace(num_classes=nms_ref.HEAD["num_classes"])

    def post_processing(batch_box_preds, batch_hm, test_cfg, post_center_range, task_id):
        captured.append((batch_box_preds.clone(), batch_hm.clone(), post_center_range.clone()))
        return head.CenterHead.post_processing(fake, batch_box_preds, batch_hm, test_cfg, post_center_range, task_id)

    fake.post_processing = post_processing
    test_cfg = Cfg(nms_ref.as_test_cfg(cfg))
    test_cfg["nms"] = Cfg(test_cfg["nms"])
    example = {"metadata": [{"token": t} for t in nms_ref.TOKENS]}
    preds = [{k: torch.from_numpy(v.copy()) for k, v in t.items()} for t in tasks]
    RECORD.clear()
    ret_list = head.CenterHead.predict(fake, example, preds, test_cfg)
    out, ok, call = {}, True, 0
    thr = np.float32(cfg["score_threshold"])
    for t, (box_preds, hm, rng_t) in enumerate(captured):
        for b in range(hm.shape[0]):
            scores, labels = torch.max(hm[b], dim=-1)
            mask = (scores > cfg["score_threshold"]) & (box_preds[b][..., :3] >= rng_t[:3]).all(1) & \
                   (box_preds[b][..., :3] <= rng_t[3:]).all(1)
            cell = torch.nonzero(mask).reshape(-1).numpy()
            bx, sc = box_preds[b][mask].numpy(), scores[mask].numpy()
            out[f"t{t}_b{b}_cell"], out[f"t{t}_b{b}_label"] = cell.astype(np.int32), labels[mask].numpy().astype(np.int32)
            out[f"t{t}_b{b}_boxes"], out[f"t{t}_b{b}_score"] = bx, sc
            # the margins
            ok = ok and bool(np.all(np.abs(scores.numpy().astype(np.float64) - np.float64(thr)) > 1e-5))
            ctr = box_preds[b][..., :3].numpy().astype(np.float64)
            faces = np.asarray(cfg["post_center_limit_range"], np.float32).astype(np.float64)
            ok = ok and bool(np.all(np.abs(ctr - faces[:3]) > 1e-3) and np.all(np.abs(ctr - faces[3:]) > 1e-3))
            ok = ok and np.unique(sc).size == sc.size
            b7 = bx[:, [0, 1, 2, 3, 4, 5, -1]]
            if cfg["circular_nms"]:
                ok = ok and circle_margin_ok(bx[:, :2], cfg["min_radius"][t])
            elif bx.shape[0]:
                o = nms_ref.order(sc)[:cfg["nms_pre_max_size"]]
                ok = ok and rotate_margin_ok(b7, o, cfg["nms_iou_threshold"], RECORD[call])
                call += 1
    assert cfg["circular_nms"] or call == len(RECORD)
    for b, ret in enumerate(ret_list):
        assert ret["metadata"]["token"] == nms_ref.TOKENS[b]
        out[f"ret{b}_boxes"], out[f"ret{b}_scores"] = ret["box3d_lidar"].numpy(), ret["scores"].numpy()
        out[f"ret{b}_labels"] = ret["label_preds"].numpy().astype(np.int64)
    return out, ok


def heads(head):
    for seed in range(200):
        out, ok = {}, True
        for run, (cfg_name, vel) in HEAD_RUNS.items():
            arrays, good = head_run(head, seed, cfg_name, vel)
            ok = ok and good
            if not ok:
                break
            out.update({f"head_{run}_{k}": v for k, v in arrays.items()})
        if not ok:
            continue
        # the NumPy restatement agrees with the reference on this input
        for run, (cfg_name, vel) in HEAD_RUNS.items():
            cfg = nms_ref.CONFIGS[cfg_name]
            tasks = nms_ref.head_maps(seed, vel)
            for t, task in enumerate(tasks):
                for b, (cell, label, boxes, score) in enumerate(nms_ref.decode(task, cfg)):
                    assert np.array_equal(cell, out[f"head_{run}_t{t}_b{b}_cell"]), (run, t, b)
                    assert np.array_equal(label, out[f"head_{run}_t{t}_b{b}_label"]), (run, t, b)
            mine = nms_ref.predict(tasks, cfg)
            for b, ret in enumerate(mine):
                want = out[f"head_{run}_ret{b}_boxes"]
                assert ret[0].shape == want.shape and np.allclose(ret[0], want, rtol=1e-5, atol=1e-6), (run, b)
                assert np.array_equal(ret[2], out[f"head_{run}_ret{b}_labels"]), (run, b)
            print(f"head {run}: seed {seed}, candidates "
                  f"{[int(out[f'head_{run}_t{t}_b{b}_cell'].size) for t in range(2) for b in range(2)]}, kept "
                  f"{[int(out[f'head_{run}_ret{b}_scores'].size) for b in range(2)]}")
        out["head_seed"] = seed
        return out
    raise RuntimeError("no head seed satisfies the margins")


def main():
    torch.set_grad_enabled(False)
    iou_cpu = gen_iou_golden.reference_iou_bev_cpu()
    torch.Tensor.cuda = lambda self, *a, **k: self          # rotate_nms_pcdet moves `keep` to the GPU
    ops, head = import_reference(iou_cpu)
    out = scene(ops, head)
    out.update(heads(head))
    path = os.path.join(HERE, "nms.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
