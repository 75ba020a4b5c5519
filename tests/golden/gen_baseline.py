#!/usr/bin/env python3
"""Generate baseline.npz from the REAL reference (jacky121298/3DAL_PyTorch): its tools/static_init.py,
tools/dynamic_init.py and tools/eval.py run, main() and all, on the seeded work dir of tests/baseline_ref.py.

The two pieces the reference does not vendor are replaced by recorders:
    fpointnet_train.provider_fpointnet   get_3d_box(size, heading, centre) stores the box and returns its number;
                                         box3d_iou(a, b) returns the IoU of tests/iou_ref.py for boxes a and b;
    pcdet...iou3d_nms_utils              boxes_iou3d_gpu(a, b) stores both arguments and returns iou_ref's 3D IoU.
So the reference's own loops form the samples, the sums, the counts, the printed lines, static/static.pkl and the mIOU
values; only recorded arrays and printed lines are stored. The generator also ASSERTS that the work dir holds every case
the tests lean on (see check_coverage) and that no number sits where the device IoU's 1e-5 could change a decision or a
printed digit.

Run only where the reference checkout exists (DAL3_REFERENCE, default /root/reference):
    python tests/golden/gen_baseline.py
"""
import contextlib
import io
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden  # noqa: E402  (the import shim of the reference's tools/)
import baseline_ref  # noqa: E402
import iou_ref  # noqa: E402

TOL = 1e-5                      # what the device IoU may differ from iou_ref by (tests/test_gpu_iou.py)


def run_main(mod, argv, returns=()):
    """mod.main() under argv -> (stdout text, {function name: its return value})"""
    got = {}
    saved = {}
    for name in returns:
        fn = saved[name] = getattr(mod, name)
        setattr(mod, name, lambda *a, _fn=fn, _n=name, **k: got.setdefault(_n, _fn(*a, **k)))
    out, old = io.StringIO(), sys.argv
    sys.argv = ["x"] + argv
    try:
        with contextlib.redirect_stdout(out):
            mod.main()
    finally:
        sys.argv = old
        for name, fn in saved.items():
            setattr(mod, name, fn)
    return out.getvalue(), got


def digits_are_safe(values):
    """every value printed with .4f is at least 2e-5 from the point where its last digit would round the other way"""
    for v in values:
        frac = (float(v) * 1e4) % 1.0
        assert abs(frac - 0.5) >= 0.2, f"{float(v)!r} prints within 2e-5 of a rounding point: pick another seed"


def check_coverage(c, annos, flav):
    """the cases the issue lists, asserted on the work dir and on what the reference made of it"""
    poses = np.array([np.reshape(f["pose"], (4, 4)) for f in c["frames"]])
    assert len({f["scene"] for f in c["frames"]}) >= 3 and np.abs(poses[:, 1, 0]).min() > 1e-3         # segments, rotation
    assert set(flav["dynamic_init"]["types"]) == {1, 2, 4} and set(flav["static_init"]["types"]) == {1, 4}
    kept = baseline_ref.drop_tracks_without_best_gt(c["static"], annos)
    assert 0 < len(kept) < len(c["static"])                                                             # some are dropped
    for name in baseline_ref.FLAVOURS:
        assert 0 < flav[name]["has_gt"].sum() < flav[name]["n_samples"]                                 # counted, not scored
    for tracks, name in ((kept, "static_init"), (c["dynamic"], "dynamic_init")):
        diff = []
        for v in tracks.values():
            for j, t in enumerate(v["token"]):
                g = baseline_ref.gt_of(annos[t], v["match"][-1])
                if g is not None:
                    pose = np.linalg.inv(np.reshape(annos[t]["veh_to_global"], [4, 4]))
                    diff.append(g[-1] - baseline_ref.transform_box(v["bbox"][j][np.newaxis], pose)[0, -1])
                    assert g.dtype == np.float32
        diff = np.array(diff)
        assert (diff < 0).any() and (diff > 0).any() and (np.abs(diff) > np.pi).any(), name
        x = (diff - baseline_ref.PER / 2) % baseline_ref.PER                    # bin edges lie at per / 2 + k per
        edge = np.minimum(x, baseline_ref.PER - x)
        assert (edge < 1e-3).any(), (name, edge.min())
        assert (np.abs(np.abs(diff % (2 * np.pi)) - np.pi) < 1e-3).any(), name
        sizes = np.concatenate([flav[name]["pred"][:, 3:6], flav[name]["label"][:, 3:6]])
        cls = np.argmin(np.linalg.norm(sizes[:, None] - baseline_ref.MEAN_SIZE[None], axis=2), axis=1)
        assert set(cls) == {0, 1, 2}, name
    ties = [v for v in kept.values() if np.sum(np.stack(v["score"]) == np.max(v["score"])) > 1]
    assert ties                                                                                         # first maximum
    near = {"in": 0, "out": 0}
    for fr in c["frames"]:
        inv = np.linalg.inv(np.reshape(fr["pose"], [4, 4]))
        for v in kept.values():
            if fr["token"] in v["token"] and baseline_ref.gt_of(annos[fr["token"]], v["match"][-1]) is not None:
                own = baseline_ref.transform_box(v["bbox"][v["token"].index(fr["token"])][np.newaxis], inv)[0]
                d = np.linalg.norm(fr["rows"][:, :3] - own[:3], axis=1)
                near["in"] += int(((d > 0.099) & (d < 0.1)).any())
                near["out"] += int(((d > 0.1) & (d < 0.101)).any())
    assert near["in"] and near["out"], near
    n_gt = [len(annos[lab["token"]]["objects"]) for lab in c["labels"].values()]
    assert min(n_gt) == 1 and max(n_gt) >= 20, n_gt


def setup():
    """import the reference's three scripts and install the recorders -> (modules, boxes, pairs)"""
    gen_golden.import_reference()
    for name in ("pcdet", "pcdet.ops", "pcdet.ops.iou3d_nms", "pcdet.ops.iou3d_nms.iou3d_nms_utils"):
        sys.modules[name] = types.ModuleType(name)          # empty stubs: tools/eval.py imports boxes_iou3d_gpu from there
        sys.modules[name].__path__ = []
    sys.modules["pcdet.ops.iou3d_nms.iou3d_nms_utils"].boxes_iou3d_gpu = None
    import static_init
    import dynamic_init
    ref_eval = gen_golden._load_file("reference_tools_eval", os.path.join(gen_golden.REF, "tools", "eval.py"))
    provider = sys.modules["fpointnet_train.provider_fpointnet"]
    boxes, pairs = [], []

    def get_3d_box(size, heading, center):
        boxes.append(np.concatenate([np.asarray(center, np.float64), np.asarray(size, np.float64), [np.float64(heading)]]))
        return len(boxes) - 1

    def box3d_iou(a, b):
        bev, v3 = iou_ref.paired(boxes[a][None], boxes[b][None])
        return v3[0], bev[0]

    def boxes_iou3d_gpu(a, b):
        assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == (1, 7) and b.shape[1] == 7
        pairs.append((a.numpy().copy(), b.numpy().copy()))
        return torch.from_numpy(iou_ref.pairwise(a.numpy(), b.numpy())[1].astype(np.float32))
    provider.get_3d_box, provider.box3d_iou = get_3d_box, box3d_iou
    ref_eval.boxes_iou3d_gpu = boxes_iou3d_gpu
    return (static_init, dynamic_init, ref_eval), boxes, pairs


def record(mods, boxes, pairs, seed):
    """the three scripts on the work dir of `seed` -> the fixture's arrays; AssertionError when the seed will not do"""
    static_init, dynamic_init, ref_eval = mods
    boxes.clear()
    pairs.clear()
    out = {"seed": np.int64(seed)}
    with tempfile.TemporaryDirectory() as tmp:
        paths, c = baseline_ref.write_work_dir(tmp, seed)
        annos = baseline_ref.annos_of(c["frames"])
        out["in_sum"] = np.float64(sum(float(np.sum(np.vstack(v["bbox"]))) for t in (c["static"], c["dynamic"]) for v in t.values())
                                   + sum(float(o["box"].astype(np.float64).sum()) for f in c["frames"] for o in f["objects"])
                                   + sum(float(f["rows"].astype(np.float64).sum()) for f in c["frames"]))
        os.makedirs(os.path.join(tmp, "static"))            # the reference fails without it
        names = ("calculate_init_iou", "calculate_static_iou")
        text_s, got_s = run_main(static_init, ["--track", paths["static"], "--infos", paths["infos"], "--det_annos",
                                               paths["det_annos"]], names)
        n_static = len(boxes)
        text_d, got_d = run_main(dynamic_init, ["--track", paths["dynamic"], "--infos", paths["infos"]], names[:1])
        n_dynamic = len(boxes) - n_static
        text_l, _ = run_main(ref_eval, ["--track", paths["static"], "--infos", paths["infos"], "--static", paths["labels"]])
        with open(os.path.join(tmp, "static", "static.pkl"), "rb") as f:
            result = pickle.load(f)
    assert all(b[6] == 0.0 for b in boxes[0::2]), "a prediction heading is not exactly 0.0"
    rec = np.stack(boxes).reshape(-1, 2, 7)
    assert n_static % 4 == 0
    parts = {"static_init": rec[:n_static // 4], "static_best": rec[n_static // 4:n_static // 2],
             "dynamic_init": rec[n_static // 2:]}
    assert len(parts["dynamic_init"]) * 2 == n_dynamic
    kept = baseline_ref.drop_tracks_without_best_gt(c["static"], annos)
    means = {"static_init": got_s["calculate_init_iou"], "static_best": got_s["calculate_static_iou"],
             "dynamic_init": got_d["calculate_init_iou"]}
    flav = {}
    for name in baseline_ref.FLAVOURS:
        s = baseline_ref.samples(c["dynamic"] if name == "dynamic_init" else kept, annos, best=(name == "static_best"))
        pred, label = parts[name][:, 0], parts[name][:, 1]
        np.testing.assert_allclose(s["pred"], pred, rtol=0, atol=1e-9)         # the restatement is the reference's recipe
        np.testing.assert_allclose(s["label"], label, rtol=0, atol=1e-9)
        bev, v3 = iou_ref.paired(pred, label)
        thr = baseline_ref.thresholds(s["types"][s["has_gt"]])
        assert np.abs(v3 - thr).min() > TOL, f"{name}: a sample within {TOL} of its threshold: pick another seed"
        n_pass = int(np.sum(v3.astype(np.float32) >= thr.astype(np.float32)))
        n = s["n_samples"]
        digits_are_safe(means[name])
        # the reference's own sums (float32 with today's NumPy) against float64 sums of the same float32 values
        want = (np.sum(bev.astype(np.float32), dtype=np.float64) / n, np.sum(v3.astype(np.float32), dtype=np.float64) / n, n_pass / n)
        assert np.allclose([float(x) for x in means[name]], want, rtol=0, atol=2e-6), (name, means[name], want)
        assert [f"{float(a):.4f}" for a in means[name]] == [f"{b:.4f}" for b in want], (name, means[name], want)
        t = s["types"][s["has_gt"]]
        flav[name] = dict(s, pred=pred, label=label)
        out.update({f"{name}_pred": pred, f"{name}_label": label, f"{name}_iou_bev": bev, f"{name}_iou_3d": v3,
                    f"{name}_has_gt": s["has_gt"], f"{name}_types": s["types"], f"{name}_best_row": s["best_row"],
                    f"{name}_n_samples": np.int64(n), f"{name}_n_pass": np.int64(n_pass),
                    f"{name}_n_type": np.array([np.sum(t == 1), np.sum(t == 2), np.sum(t == 4), np.sum(~np.isin(t, [1, 2, 4]))], np.int64),
                    f"{name}_means": np.array([float(x) for x in means[name]])})
    check_coverage(c, annos, flav)
    out["static_lines"], out["dynamic_lines"], out["labels_lines"] = np.array(text_s), np.array(text_d), np.array(text_l)

    # static/static.pkl against the sorted input
    before = sorted(c["det_annos"], key=lambda d: d["frame_id"])
    assert [d["frame_id"] for d in result] == [d["frame_id"] for d in before]
    assert all(list(d.keys()) == list(b.keys()) for d, b in zip(result, before))
    out["pkl_frame_ids"] = np.array([d["frame_id"] for d in result])
    out["pkl_keys"] = np.array(list(result[0].keys()))
    out["pkl_offsets"] = np.cumsum([0] + [len(d["boxes_lidar"]) for d in result]).astype(np.int64)
    out["pkl_boxes"] = np.concatenate([d["boxes_lidar"] for d in result]).astype(np.float32)
    out["pkl_score"] = np.concatenate([d["score"] for d in result]).astype(np.float32)
    changed = np.concatenate([np.any(d["boxes_lidar"] != b["boxes_lidar"], axis=1) | (d["score"] != b["score"])
                              for d, b in zip(result, before)])
    out["pkl_rewritten"] = changed
    n_scored = int(flav["static_best"]["has_gt"].sum())
    assert 0 < changed.sum() < n_scored, "no frame where two samples hit the same detection row"

    # tools/eval.py: per labels entry the track query, then the static query, each against the frame's GT boxes
    assert len(pairs) == 2 * len(c["labels"])
    for (qa, ga), (qb, gb) in zip(pairs[0::2], pairs[1::2]):
        assert np.array_equal(ga, gb)
    out["lab_ids"] = np.array(list(c["labels"].keys()))
    out["lab_query_track"] = np.concatenate([p[0] for p in pairs[0::2]])
    out["lab_query_static"] = np.concatenate([p[0] for p in pairs[1::2]])
    out["lab_gt_offsets"] = np.cumsum([0] + [len(p[1]) for p in pairs[0::2]]).astype(np.int64)
    out["lab_gt"] = np.concatenate([p[1] for p in pairs[0::2]])
    iou_t = np.array([iou_ref.pairwise(p[0], p[1])[1].astype(np.float32).max() for p in pairs[0::2]], np.float32)
    iou_s = np.array([iou_ref.pairwise(p[0], p[1])[1].astype(np.float32).max() for p in pairs[1::2]], np.float32)
    out["lab_iou_track"], out["lab_iou_static"] = iou_t, iou_s
    out["lab_miou"] = np.array([np.mean(list(iou_t)), np.mean(list(iou_s))], np.float32)
    assert f"mIOU of track: {out['lab_miou'][0]}" in text_l and f"mIOU of static: {out['lab_miou'][1]}" in text_l
    print(text_s + text_d + text_l)
    print(f"baseline: {[(k, int(flav[k]['has_gt'].sum()), flav[k]['n_samples']) for k in flav]} scored/all samples, "
          f"{int(changed.sum())} rewritten rows, {len(c['labels'])} labels")
    return out


def main():
    """without arguments: record baseline_ref.SEED. --search N: try N seeds from baseline_ref.SEED on and name the first
    whose numbers keep clear of every threshold and rounding point (put it into baseline_ref.SEED, then run again)."""
    mods, boxes, pairs = setup()
    if len(sys.argv) == 3 and sys.argv[1] == "--search":
        for seed in range(baseline_ref.SEED, baseline_ref.SEED + int(sys.argv[2])):
            try:
                record(mods, boxes, pairs, seed)
            except AssertionError as e:
                print(f"seed {seed}: {str(e).splitlines()[0] if str(e) else 'coverage'}")
                continue
            print(f"seed {seed} will do")
            return
        raise SystemExit("no seed found")
    out = record(mods, boxes, pairs, baseline_ref.SEED)
    np.savez_compressed(os.path.join(HERE, "baseline.npz"), **out)
    print(f"{os.path.getsize(os.path.join(HERE, 'baseline.npz'))} bytes")


if __name__ == "__main__":
    main()
