#!/usr/bin/env python3
"""Generate train_metrics.npz from the REAL reference (jacky121298/3DAL_PyTorch):

    decode   the reference's own compute_box3d_iou (tools/utils.py:81-103) on seeded head outputs and labels, with the
             un-vendored fpointnet_train.provider_fpointnet replaced by a recorder: its get_3d_box(size, heading,
             centre) calls are stored, i.e. the two boxes the reference hands to the geometry for every item. The
             inputs include heading-score ties, residuals that take the angle just above pi, every size class and
             two-way size-score ties; float32 arrays as the drivers pass them (.cpu().numpy() of float32 tensors);
    split    the train / validation keys of the reference's static_train.preprocessing and dynamic_train.preprocessing
             after fixSeed(10922081), on a synthetic track set written here (scores, tokens, the matched name, and
             annotation pickles in which some best-score frames lack that name). The set is rebuilt from the stored
             keys, scores and flags by the test.

Run only where the reference checkout exists (DAL3_REFERENCE, default /root/reference):
    python tests/golden/gen_train_metrics.py
"""
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402  (the import shim of the reference's tools/)

B = 96
N_TRACKS, N_FRAMES = 23, 6


def decode_inputs(seed=4242):
    """the ten compute_box3d_iou arrays, float32 / int64 as the drivers pass them"""
    rng = np.random.default_rng(seed)
    f = np.float32
    center = rng.normal(0, 3, (B, 3)).astype(f)
    hs = rng.normal(0, 1, (B, 12)).astype(f)
    hs[:8, 3] = hs[:8, 7] = hs[:8].max(1) + 1          # ties: the first index wins
    hs[8:12] = 0.5                                     # all twelve tied
    hr = rng.normal(0, 0.3, (B, 12)).astype(f)
    top = np.argmax(hs, 1)
    hr[np.arange(12, 24), top[12:24]] = 0.02           # predicted class 6 + a small residual: just above pi
    hs[12:24, :] = 0
    hs[12:24, 6] = 1
    ss = rng.normal(0, 1, (B, 3)).astype(f)
    ss[24:48] = 0
    ss[24:48, np.arange(24) % 3] = 1                   # every size class
    ss[48:52, 1] = ss[48:52, 2] = ss[48:52].max(1) + 1  # two-way tie: class 1
    sr = rng.normal(0, 0.2, (B, 3, 3)).astype(f)
    cl = rng.normal(0, 3, (B, 3)).astype(f)
    hcl = rng.integers(0, 12, B).astype(np.int64)
    hcl[:12] = 6
    hrl = rng.normal(0, 0.25, B).astype(f)
    hrl[:12] = np.abs(hrl[:12]) + 1e-3                 # label angles just above pi too
    scl = (np.arange(B) % 3).astype(np.int64)
    srl = rng.normal(0, 0.2, (B, 3)).astype(f)
    return center, hs, hr, ss, sr, cl, hcl, hrl, scl, srl


def track_set(seed=77):
    """keys, per-frame scores and per-frame 'has the matched annotation' flags of the split's track set"""
    rng = np.random.default_rng(seed)
    keys = np.array([f"trk{k:03d}_{int(rng.integers(1000))}" for k in range(N_TRACKS)])
    scores = rng.uniform(0, 1, (N_TRACKS, N_FRAMES)).astype(np.float32)
    has_gt = rng.uniform(0, 1, (N_TRACKS, N_FRAMES)) > 0.3
    return keys, scores, has_gt


def write_track_set(root, keys, scores, has_gt):
    """-> (track dict, infos {token: info}) in the reference's schema, annotation pickles under root"""
    track, infos = {}, {}
    for k, key in enumerate(keys):
        tokens = [f"{key}_f{j}" for j in range(N_FRAMES)]
        track[str(key)] = {"score": [np.float32(s) for s in scores[k]], "token": tokens, "match": ["x", f"obj_{key}"]}
        for j, tok in enumerate(tokens):
            objs = [{"name": "other", "box": np.zeros(9, np.float32)}]
            if has_gt[k, j]:
                objs.append({"name": f"obj_{key}", "box": np.ones(9, np.float32)})
            path = os.path.join(root, tok + ".pkl")
            with open(path, "wb") as fh:
                pickle.dump({"veh_to_global": np.eye(4).reshape(16), "objects": objs}, fh)
            infos[tok] = {"anno_path": path, "token": tok}
    return track, infos


def main():
    _, _, _, _, ut = gen_golden.import_reference()
    import static_train
    import dynamic_train
    provider = sys.modules["fpointnet_train.provider_fpointnet"]
    boxes = []
    provider.get_3d_box = lambda size, heading, center: boxes.append(
        np.concatenate([np.asarray(center, np.float64), np.asarray(size, np.float64), [np.float64(heading)]])) or len(boxes) - 1
    provider.box3d_iou = lambda a, b: (0.0, 0.0)
    inputs = decode_inputs()
    ut.compute_box3d_iou(*inputs)
    boxes = np.stack(boxes).reshape(B, 2, 7)
    out = {name: arr for name, arr in zip(("center", "heading_scores", "heading_residuals", "size_scores",
                                            "size_residuals", "center_label", "heading_class_label",
                                            "heading_residual_label", "size_class_label", "size_residual_label"), inputs)}
    out["pred_box"], out["label_box"] = boxes[:, 0], boxes[:, 1]
    keys, scores, has_gt = track_set()
    out.update(track_keys=keys, track_scores=scores, track_has_gt=has_gt)
    with tempfile.TemporaryDirectory() as tmp:
        track, infos = write_track_set(tmp, keys, scores, has_gt)
        ut.fixSeed(seed=10922081)
        tr, va = static_train.preprocessing(dict(track), infos)
        out["static_train_keys"], out["static_val_keys"] = np.array(list(tr)), np.array(list(va))
        ut.fixSeed(seed=10922081)
        tr, va = dynamic_train.preprocessing(dict(track))
        out["dynamic_train_keys"], out["dynamic_val_keys"] = np.array(list(tr)), np.array(list(va))
    np.savez_compressed(os.path.join(HERE, "train_metrics.npz"), **out)
    print(f"train_metrics: {B} decoded pairs; static split {len(out['static_train_keys'])}/{len(out['static_val_keys'])}, "
          f"dynamic split {len(out['dynamic_train_keys'])}/{len(out['dynamic_val_keys'])}")


if __name__ == "__main__":
    main()
