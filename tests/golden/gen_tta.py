#!/usr/bin/env python3
"""Generate tests/golden/tta.npz from the REAL reference (jacky121298/3DAL_PyTorch): `CenterHead.predict` with
`test_cfg.double_flip` (det3d/models/bbox_heads/center_head.py:318-414) on tests/tta_ref.py's seeded head maps (8 maps of
12 x 20 per task: two merged samples, four independent random views each, so that a wrong sign, view or mirrored index
shows in every cell and a row / column mix-up cannot cancel), and `DoubleFlip` (det3d/datasets/pipelines/test_aug.py) on
a small seeded sweep.

Run only where the reference checkout exists (DAL3_REFERENCE, default /root/reference):
    python tests/golden/gen_tta.py

The reference is imported as gen_nms.py imports it (stub modules around center_head.py, the CPU IoU behind `nms_gpu`), and
`post_processing` is captured as there: what is recorded per (task, merged sample) are the survivors of the reference's own
masks on the merged maps, and the kept rows of `predict`.

The margins are conditions, asserted on the seed that is used: no merged score within 1e-5 of the threshold, no centre
within 1e-3 m of a face of the range, unique scores per segment, gen_nms.py's IoU and radius margins, and between 25 % and
80 % of the cells surviving per (task, sample) (under "small", whose range is there to bite, of the cells above the score
threshold). The restatement (tta_ref.merge_decode / predict) must reproduce the reference: cells and labels exactly,
x / y / z / vel bit for bit (sums of four and one division in torch's order), the libm columns to rtol 1e-5.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gen_iou_golden  # noqa: E402
import gen_nms  # noqa: E402
import nms_ref  # noqa: E402
import tta_ref  # noqa: E402

NUM_CLASSES = tta_ref.HEAD["num_classes"]
SAMPLES = tta_ref.HEAD["B"] // 4


def head_run(head, seed, cfg_name, vel):
    """-> (arrays, ok)"""
    cfg = nms_ref.CONFIGS[cfg_name]
    tasks = tta_ref.head_maps(seed, vel)
    captured = []
    fake = types.SimpleNamespace(num_classes=NUM_CLASSES)

    def post_processing(batch_box_preds, batch_hm, test_cfg, post_center_range, task_id):
        captured.append((batch_box_preds.clone(), batch_hm.clone(), post_center_range.clone()))
        return head.CenterHead.post_processing(fake, batch_box_preds, batch_hm, test_cfg, post_center_range, task_id)

    fake.post_processing = post_processing
    test_cfg = gen_nms.Cfg(nms_ref.as_test_cfg(cfg), double_flip=True)
    test_cfg["nms"] = gen_nms.Cfg(test_cfg["nms"])
    example = {"metadata": [{"token": t} for t in tta_ref.TOKENS]}
    preds = [{k: torch.from_numpy(v.copy()) for k, v in t.items()} for t in tasks]
    gen_nms.RECORD.clear()
    ret_list = head.CenterHead.predict(fake, example, preds, test_cfg)
    assert len(ret_list) == SAMPLES
    out, ok, call = {}, True, 0
    thr = np.float32(cfg["score_threshold"])
    for t, (box_preds, hm, rng_t) in enumerate(captured):
        assert hm.shape[0] == SAMPLES
        for b in range(SAMPLES):
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
            # ("small" exists so that the range bites: there the score mask alone is held to the 25 - 80 %)
            live = scores > cfg["score_threshold"] if cfg_name == "small" else mask
            ok = ok and 0.25 <= float(live.float().mean()) <= 0.80
            b7 = bx[:, [0, 1, 2, 3, 4, 5, -1]]
            if cfg["circular_nms"]:
                ok = ok and gen_nms.circle_margin_ok(bx[:, :2], cfg["min_radius"][t])
            elif bx.shape[0]:
                o = nms_ref.order(sc)[:cfg["nms_pre_max_size"]]
                ok = ok and gen_nms.rotate_margin_ok(b7, o, cfg["nms_iou_threshold"], gen_nms.RECORD[call])
                call += 1
    assert cfg["circular_nms"] or call == len(gen_nms.RECORD)
    for b, ret in enumerate(ret_list):
        assert ret["metadata"]["token"] == tta_ref.TOKENS[4 * b]            # every fourth: the sample's unflipped view
        out[f"ret{b}_boxes"], out[f"ret{b}_scores"] = ret["box3d_lidar"].numpy(), ret["scores"].numpy()
        out[f"ret{b}_labels"] = ret["label_preds"].numpy().astype(np.int64)
    return out, ok


def heads(head):
    for seed in range(200):
        out, ok = {}, True
        for run, (cfg_name, vel) in tta_ref.RUNS.items():
            arrays, good = head_run(head, seed, cfg_name, vel)
            ok = ok and good
            if not ok:
                break
            out.update({f"tta_{run}_{k}": v for k, v in arrays.items()})
        if not ok:
            continue
        # the NumPy restatement reproduces the reference on this input
        for run, (cfg_name, vel) in tta_ref.RUNS.items():
            cfg = nms_ref.CONFIGS[cfg_name]
            tasks = tta_ref.head_maps(seed, vel)
            exact = [0, 1, 2] + ([6, 7] if vel else [])
            for t, task in enumerate(tasks):
                for b, (cell, label, boxes, score) in enumerate(tta_ref.merge_decode(task, cfg)):
                    key = f"tta_{run}_t{t}_b{b}_"
                    assert np.array_equal(cell, out[key + "cell"]) and np.array_equal(label, out[key + "label"]), key
                    want = out[key + "boxes"]
                    assert np.array_equal(boxes[:, exact].view(np.uint32), want[:, exact].view(np.uint32)), key
                    np.testing.assert_allclose(boxes, want, rtol=1e-5, atol=0)
                    np.testing.assert_allclose(score, out[key + "score"], rtol=1e-5, atol=0)
            for b, ret in enumerate(tta_ref.predict(tasks, cfg)):
                want = out[f"tta_{run}_ret{b}_boxes"]
                assert ret[0].shape == want.shape and want.shape[0] > 0, (run, b)
                np.testing.assert_allclose(ret[0], want, rtol=1e-5, atol=0)
                assert np.array_equal(ret[2], out[f"tta_{run}_ret{b}_labels"]), (run, b)
            cells = tta_ref.HEAD["H"] * tta_ref.HEAD["W"]
            print(f"tta {run}: seed {seed}, survivors "
                  f"{[round(out[f'tta_{run}_t{t}_b{b}_cell'].size / cells, 2) for t in range(2) for b in range(SAMPLES)]}, kept "
                  f"{[int(out[f'tta_{run}_ret{b}_scores'].size) for b in range(SAMPLES)]}")
        out["tta_seed"] = seed
        return out
    raise RuntimeError("no seed satisfies the margins")


def double_flip():
    """test_aug.py's DoubleFlip on tta_ref.sweep(): its three arrays"""
    registry = types.SimpleNamespace(register_module=lambda cls: cls)
    for name in ("det3d.datasets", "det3d.datasets.pipelines"):
        gen_nms._stub(name)
    gen_nms._stub("det3d.datasets.registry", PIPELINES=registry)
    gen_nms._stub("det3d.datasets.pipelines.compose", Compose=None)
    mod = gen_nms._load_file("det3d.datasets.pipelines.test_aug", "det3d/datasets/pipelines/test_aug.py")
    pts = tta_ref.sweep()
    res, _ = mod.DoubleFlip()({"lidar": {"points": pts.copy()}}, None)
    assert np.array_equal(res["lidar"]["points"].view(np.uint32), pts.view(np.uint32))
    views = [res["lidar"][k] for k in ("yflip_points", "xflip_points", "double_flip_points")]
    mine, off = tta_ref.flip4_points(pts, [0, pts.shape[0]])
    for v, want in enumerate([pts] + views):
        assert np.array_equal(mine[off[v]:off[v + 1]].view(np.uint32), want.view(np.uint32)), v
    return {"flip_yflip": views[0], "flip_xflip": views[1], "flip_double": views[2],
            "flip_sum": float(pts.astype(np.float64).sum())}


def main():
    torch.set_grad_enabled(False)
    iou_cpu = gen_iou_golden.reference_iou_bev_cpu()
    torch.Tensor.cuda = lambda self, *a, **k: self          # rotate_nms_pcdet moves `keep` to the GPU
    ops, head = gen_nms.import_reference(iou_cpu)
    out = heads(head)
    out.update(double_flip())
    path = os.path.join(HERE, "tta.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
