#!/usr/bin/env python3
"""Generate the rotated-box IoU fixtures from the REAL reference (jacky121298/3DAL_PyTorch):

    iou_ref_pairs.npz  the reference's own CPU IoU (det3d/ops/iou3d_nms/src/iou3d_cpu.cpp, boxes_iou_bev_cpu) on the
                       ~20k pairs of tests/iou_ref.py fixture_pairs() (random near-overlapping pairs plus designed
                       cases; rebuilt from their seed where used, only a checksum stored): its BEV IoU, and the 3D IoU
                       derived from it as boxes_iou3d_gpu forms it (overlap = iou (A_a + A_b) / (1 + iou), times the
                       z overlap, over the union of the volumes; its to_pcdet mirror leaves IoU unchanged);
    eval_metrics.npz   the reference's real `postprocessing` (tools/static_eval.py, tools/dynamic_eval.py) on a
                       synth.segment_files segment, with compute_box3d_iou replaced by a recorder that rebuilds the
                       two boxes with the reference's own class2angle / class2size and scores them with
                       tests/iou_ref.py (the un-vendored fpointnet geometry is the one substitution): per-sample boxes,
                       types, IoUs and the three numbers the run logs.

Run only where the reference checkout exists (DAL3_REFERENCE, default /root/reference):
    python tests/golden/gen_iou_golden.py

The C++ source is compiled from the reference checkout into a temporary directory outside the tree (stub cuda.h /
cuda_runtime_api.h: the CPU file includes them but uses nothing from them); only its outputs are stored.
"""
import importlib
import logging
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
synth = importlib.import_module("3dal_pytorch_amd.synth")
ev = importlib.import_module("3dal_pytorch_amd.eval")
import gen_golden  # noqa: E402  (the import shim of the reference's tools/)
import iou_ref  # noqa: E402

REF = gen_golden.REF
SEGMENT = dict(seed=61, n_frames=24, n_tracks=12)          # the eval fixture's synth.segment_files arguments


def reference_iou_bev_cpu():
    from torch.utils.cpp_extension import load_inline
    src_dir = os.path.join(REF, "det3d", "ops", "iou3d_nms", "src")
    build = tempfile.mkdtemp(prefix="iou3d_cpu_ref_")
    stub = os.path.join(build, "stub")
    os.makedirs(stub)
    with open(os.path.join(stub, "cuda.h"), "w") as f:
        f.write("#define __device__\n")
    open(os.path.join(stub, "cuda_runtime_api.h"), "w").close()
    with open(os.path.join(src_dir, "iou3d_cpu.cpp")) as f:
        source = f.read()
    mod = load_inline("iou3d_cpu_ref", cpp_sources=[source], functions=["boxes_iou_bev_cpu"],
                      extra_include_paths=[stub, src_dir], build_directory=build, verbose=False)
    return mod.boxes_iou_bev_cpu


def ref_pairs(out_dir):
    fn = reference_iou_bev_cpu()
    a64, b64, nd = iou_ref.fixture_pairs()               # float32 values: what the reference's fp32 code sees
    a32, b32 = torch.from_numpy(a64.astype(np.float32)), torch.from_numpy(b64.astype(np.float32))
    bev = np.empty(a64.shape[0], np.float32)
    for k in range(a64.shape[0]):                      # paired: one 1x1 call per pair
        o = torch.zeros((1, 1), dtype=torch.float32)
        fn(a32[k:k + 1].contiguous(), b32[k:k + 1].contiguous(), o)
        bev[k] = o.item()
    area_a, area_b = a64[:, 3] * a64[:, 4], b64[:, 3] * b64[:, 4]
    ov = bev.astype(np.float64) * (area_a + area_b) / (1 + bev.astype(np.float64))
    zo = np.clip(np.minimum(a64[:, 2] + a64[:, 5] / 2, b64[:, 2] + b64[:, 5] / 2)
                 - np.maximum(a64[:, 2] - a64[:, 5] / 2, b64[:, 2] - b64[:, 5] / 2), 0, None)
    o3 = ov * zo
    v3 = o3 / np.maximum(area_a * a64[:, 5] + area_b * b64[:, 5] - o3, 1e-6)
    # the boxes are rebuilt from iou_ref.fixture_pairs() where the fixture is used; only their checksum is stored
    np.savez_compressed(os.path.join(out_dir, "iou_ref_pairs.npz"), iou_bev=bev, iou_3d=v3.astype(np.float32),
                        n_designed=nd, in_sum=a64.sum() + b64.sum())
    mine = iou_ref.paired(a64, b64)[0]
    d = np.abs(mine - bev)
    print(f"iou_ref_pairs: {a64.shape[0]} pairs, median |d| {np.median(d):.2e}, within 1e-5 {np.mean(d <= 1e-5):.4f}, "
          f"max {d.max():.2e}")


def eval_metrics(out_dir):
    _, _, se, de, ut = gen_golden.import_reference()
    calls = []

    def recorder(center_pred, heading_logits, heading_residuals, size_logits, size_residuals, center_label,
                 heading_class_label, heading_residual_label, size_class_label, size_residual_label):
        """compute_box3d_iou (tools/utils.py:81-103) with its box reconstruction kept and its geometry replaced"""
        hc = int(np.argmax(heading_logits, 1)[0])
        sc = int(np.argmax(size_logits, 1)[0])
        pred = np.concatenate([np.asarray(center_pred[0], np.float64), ut.class2size(sc, size_residuals[0, sc, :]),
                               [ut.class2angle(hc, heading_residuals[0, hc], ut.NUM_HEADING_BIN)]])
        gt = np.concatenate([np.asarray(center_label[0], np.float64),
                             ut.class2size(size_class_label[0], size_residual_label[0]),
                             [ut.class2angle(heading_class_label[0], heading_residual_label[0], ut.NUM_HEADING_BIN)]])
        vb, v3 = iou_ref.paired(pred[None], gt[None])
        calls.append((pred, gt, float(vb[0]), float(v3[0])))
        return vb.astype(np.float32), v3.astype(np.float32)

    se.compute_box3d_iou = de.compute_box3d_iou = recorder
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths, tracks, poses, dets, has_gt = synth.segment_files(tmp, **SEGMENT)
        infos = ut.reorganize_info(pickle.load(open(paths["infos"], "rb")))
        det_annos = ev.sort_detections(pickle.load(open(paths["det_annos"], "rb")))
        token2idx = ev.token_to_det_index(infos, det_annos, ev.Annos(infos))
        for head, mod in (("static", se), ("dynamic", de)):
            track = pickle.load(open(paths[head], "rb"))
            if head == "static":
                track = se.preprocessing(track, infos)
            tl = list(track.values())
            if head == "static":                       # each track's best box in its best frame, perturbed
                base = []
                for v in tl:
                    best = int(np.argmax(np.stack(v["score"])))
                    inv = np.linalg.inv(np.reshape(poses[v["token"][best]], [4, 4]))
                    base.append(se.transform_box(np.asarray(v["bbox"][best], np.float64)[None], inv)[0])
            else:                                      # every track-frame's box in its own frame, perturbed
                base = [se.transform_box(np.asarray(v["bbox"][j], np.float64)[None],
                                         np.linalg.inv(np.reshape(poses[t], [4, 4])))[0]
                        for v in tl for j, t in enumerate(v["token"])]
            base = np.stack(base)
            for attempt in range(100):
                rng = np.random.default_rng(1000 * (head == "dynamic") + attempt)
                final = base.copy()
                final[:, :2] += rng.normal(0, 0.06, (len(final), 2)) * final[:, 3:5]
                final[:, 2] += rng.normal(0, 0.08, len(final))
                final[:, 3:6] *= 0.9 * rng.uniform(0.93, 1.07, (len(final), 3))     # the annotations are 0.9 x the track box
                final[:, 6] += rng.normal(0, 0.06, len(final))
                calls.clear()
                res = mod.postprocessing(pickle.loads(pickle.dumps(track)), infos, token2idx, final.copy(),
                                         [dict(d, boxes_lidar=d["boxes_lidar"].copy()) for d in det_annos],
                                         os.path.join(tmp, f"res_{head}.pkl"), logging.getLogger("gen_iou"))
                v3 = np.array([c[3] for c in calls])
                if np.min(np.abs(np.concatenate([v3 - 0.5, v3 - 0.7]))) > 1e-4:
                    break
            else:
                raise RuntimeError("no perturbation keeps every 3D IoU away from the thresholds")
            iou2d, iou3d, acc = (float(x) for x in res[:3])
            s2d = float(np.sum(np.array([c[2] for c in calls], np.float32).astype(np.float64)))
            n_samples = s2d / iou2d
            assert abs(n_samples - round(n_samples)) < 1e-3, n_samples   # the sums run in float32 there
            annos = ev.Annos(infos)                    # the type of every sample, in the loop's order (an input)
            types = np.array([v["type"][j] for v in tl for j, t in enumerate(v["token"])
                              if annos.gt_box(t, v["match"][-1]) is not None])
            assert len(types) == len(calls)
            out.update({f"{head}_final": final, f"{head}_pred": np.stack([c[0] for c in calls]),
                        f"{head}_gt": np.stack([c[1] for c in calls]), f"{head}_types": types,
                        f"{head}_iou_bev": np.array([c[2] for c in calls]), f"{head}_iou_3d": v3,
                        f"{head}_iou2d": iou2d, f"{head}_iou3d": iou3d, f"{head}_acc": acc,
                        f"{head}_n_samples": int(round(n_samples)), f"{head}_attempt": attempt})
            print(f"eval_metrics {head}: {len(calls)} samples of {int(round(n_samples))}, IoU 2D/3D {iou2d:.4f}/{iou3d:.4f}, "
                  f"accuracy {acc:.4f}, 3D IoU range {v3.min():.3f}..{v3.max():.3f} (attempt {attempt})")
    np.savez_compressed(os.path.join(out_dir, "eval_metrics.npz"), **out, segment_seed=SEGMENT["seed"],
                        segment_n_frames=SEGMENT["n_frames"], segment_n_tracks=SEGMENT["n_tracks"])


def main():
    torch.set_grad_enabled(False)
    ref_pairs(HERE)
    eval_metrics(HERE)


if __name__ == "__main__":
    main()
