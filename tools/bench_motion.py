#!/usr/bin/env python3
"""The motion-state run at the size of a Waymo split (tools/bench_track.py's: 200 sequences x 198 frames x 100-300
objects, 40 % of them parked, the others moving at up to 10 m/s, so both classes are present and the slow movers overlap
the parked ones). The tracker's result is the input. Times, on the current GPU:
  group / features / classify   dal3_group_by_key, dal3_track_features, dal3_motion_classify alone (HIP events around
                                each call, median of --reps after a warm-up), with the bytes each must move and the
                                rate that gives against the 6.3 TB/s a copy reaches on this GPU
  call                          group -> features -> classify -> MotionResult.tracks(): the kernels, the downloads, the
                                per-track slicing on the host (wall clock, ends in a synchronise)
  cpu                           the restated CPU path on --cpu_seqs sequences: track.regroup on their trackData dicts +
                                NumPy's trackFeature expressions per track, scaled to the split; its features are
                                checked against the kernel's
  svm_fit                       motion.fit_linear_svm on the kept tracks' features with the GT rule's labels (host)
One JSON line; --out writes it to a file.
    python tools/bench_motion.py [--seqs 200 --frames 198 --reps 20 --out profiles/bench_motion.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
trk = importlib.import_module("3dal_pytorch_amd.track")
motion = importlib.import_module("3dal_pytorch_amd.motion")
HBM_COPY_BYTES_PER_S = 6.3e12


def split_input(seed, S, F):
    """flat tracker inputs + per detection the global centre (at 1e4 m), and per object the GT rule's static flag"""
    rng = np.random.default_rng(seed)
    ct, tr, lab, sc, counts, starts, obj, static = [], [], [], [], [], [], [], []
    n_obj = 0
    for s in range(S):
        starts.append(len(counts))
        n = int(rng.integers(100, 301))
        p, L = rng.uniform(-75, 75, (n, 2)) + [1.2e4, -0.9e4], rng.integers(0, 3, n)
        speed = np.where(rng.uniform(0, 1, n) < 0.4, 0.0, rng.uniform(0, 10, n))
        th = rng.uniform(-np.pi, np.pi, n)
        v = speed[:, None] * np.stack([np.cos(th), np.sin(th)], 1)
        static.append((speed * 0.1 * (F - 1) < 1) & (speed < 1))
        for f in range(F):
            idx = np.nonzero(rng.uniform(0, 1, n) > 0.1)[0]
            idx = idx[rng.permutation(len(idx))]
            ct.append(p[idx] + v[idx] * 0.1 * f + rng.normal(0, 0.03, (len(idx), 2)))
            tr.append(-v[idx] * (0.0 if f == 0 else 0.1))
            lab.append(L[idx])
            sc.append(rng.uniform(0.76, 1.0, len(idx)).astype(np.float32))
            obj.append(n_obj + idx)
            counts.append(len(idx))
        n_obj += n
    fo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return (np.concatenate(ct), np.concatenate(tr), np.concatenate(lab).astype(np.int32), np.concatenate(sc), fo,
            np.asarray(starts + [len(counts)], np.int64), np.concatenate(obj).astype(np.int32), np.concatenate(static))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def cpu_path(frames_out, fo, f_end, centre, typ, score, n_points, match):
    """trackData dicts of the first frames -> track.regroup -> trackFeature's expressions per track"""
    td = {}
    for f in range(f_end):
        b, t = frames_out[f]
        d = fo[f] + b
        td[f"f{f}"] = {"id": [int(x) for x in t], "type": list(typ[d]), "bbox": list(centre[d]), "score": list(score[d]),
                       "point": list(n_points[d]), "match": list(match[d])}
    t0 = time.perf_counter()
    tracks = trk.regroup(td)
    t_regroup = time.perf_counter() - t0
    t0 = time.perf_counter()
    feats = {}
    for tid, o in tracks.items():
        bbox = np.array(o["bbox"])
        keep = not (o["match"][-1] < 0 or bbox.shape[0] < 7 or o["type"][0] == 2 or sum(o["point"]) == 0)
        feats[tid] = (keep, np.linalg.norm(bbox[0, :3] - bbox[-1, :3]), np.linalg.norm(np.var(bbox[:, :3], axis=0)))
    return t_regroup * 1e3, (time.perf_counter() - t0) * 1e3, feats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=200)
    ap.add_argument("--frames", type=int, default=198)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu_seqs", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    ct, tr, lab, sc, fo, so, obj, obj_static = split_input(7, a.seqs, a.frames)
    K = len(lab)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    b = trk.TrackInputs.__new__(trk.TrackInputs)
    b.counts, b.seq_offsets = np.diff(fo), so
    res = trk.track_sequences(seq_offsets=t(so), frame_offsets=t(fo), ct=t(ct), tracking=t(tr), label=t(lab), score=t(sc),
                              capacity=b.capacity(3))
    ids = res.total()
    # per-detection arrays -> per-entry arrays (by output position), on the device
    rng = np.random.default_rng(3)
    centre = np.concatenate([ct, rng.normal(1.5, 0.02, (K, 1))], 1)
    typ = np.asarray([1, 2, 4], np.int32)[lab]
    n_points = rng.integers(0, 300, K).astype(np.int32)
    det = motion.detection_index(res)
    e_centre, e_type, e_score = t(centre)[det].contiguous(), t(typ)[det].contiguous(), t(sc)[det].contiguous()
    e_points, e_match = t(n_points)[det].contiguous(), t(obj)[det].contiguous()
    model = (np.array([-2.0, -0.5]), 1.5)
    out = {}
    for name, cap in (("capacity_ids", ids), ("capacity_default", None)):
        run_g = lambda: motion.group_tracks(res, capacity=cap)   # noqa: E731
        groups = run_g()
        run_f = lambda: motion.track_features(groups, e_centre, e_type, e_score, e_points, e_match)   # noqa: E731
        feats = run_f()
        run_c = lambda: motion.classify(feats.feature, feats.keep, model)   # noqa: E731
        run_c()
        for fn in (run_g, run_f, run_c):                    # warm-up
            fn()
        torch.cuda.synchronize()
        E, T = groups.E, groups.T
        n_in = int(groups.group_start[-1].item())
        passes = 1 + (max(T, 1).bit_length() - 1) // 8
        byt = {"group": 12 * E + passes * 20 * E - 4 * E + 8 * (T + 1),     # keys in / out, per pass hist + scatter
               "features": 3 * 4 * n_in + 8 * n_in + 2 * 24 * n_in + 8 * (T + 1) + 37 * T,
               "classify": 2 * 17 * T + 9 * T + 4 * T}
        rec = {"T": T, "E": E, "entries": n_in, "radix_passes": passes}
        for key, fn in (("group", run_g), ("features", run_f), ("classify", run_c)):
            med, lo, hi = timed(fn, a.reps)
            rec[key] = {"ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes": int(byt[key]),
                        "TB_per_s": round(byt[key] / (med * 1e-3) / 1e12, 3),
                        "share_of_copy_rate": round(byt[key] / (med * 1e-3) / HBM_COPY_BYTES_PER_S, 3)}
        out[name] = rec
    # the whole call, host work included
    scores = [sc[fo[f]:fo[f + 1]] for f in range(len(fo) - 1)]

    def call():
        r = motion.motion_state(res, e_centre, e_type, e_score, e_points, e_match, model, capacity=ids)
        return r, r.tracks(scores)
    call()
    t0 = time.perf_counter()
    for _ in range(3):
        r, tracks = call()
    t_call = (time.perf_counter() - t0) / 3 * 1e3
    # the restated CPU path on the first sequences, checked against the kernel
    f_end = int(so[a.cpu_seqs])
    frames_out = res.frames()
    t_regroup, t_feat, cpu = cpu_path(frames_out, fo, f_end, centre, typ, sc, n_points, obj)
    keep, feat = r.features.keep.cpu().numpy(), r.features.feature.cpu().numpy()
    ok = all(bool(keep[tid - 1]) == k and (not k or np.allclose(feat[tid - 1], [d, v], rtol=1e-9, atol=0)) for tid, (k, d, v) in cpu.items())
    # the SVM on the kept tracks: label = the GT rule's flag of the matched object
    kept = keep.astype(bool)
    X = feat[kept]
    Y = obj_static[r.features.match_last.cpu().numpy()[kept]].astype(np.int64)
    info = {}
    w, bias = motion.fit_linear_svm(X, Y, info=info)
    acc = float(np.mean(((X @ w + bias) > 0) == (Y == 1)))
    rec = {"bench": "motion", "device": torch.cuda.get_device_name(0), "sequences": a.seqs, "frames": int(len(fo) - 1),
           "detections": K, "ids": ids, "tracks_out": len(tracks), "kernels": out, "reps": a.reps,
           "call_ms": round(t_call, 1),
           "cpu": {"sequences": a.cpu_seqs, "regroup_ms_per_sequence": round(t_regroup / a.cpu_seqs, 1),
                   "track_feature_ms_per_sequence": round(t_feat / a.cpu_seqs, 1),
                   "split_estimate_ms": round((t_regroup + t_feat) / a.cpu_seqs * a.seqs, 0), "equal_to_kernel": bool(ok)},
           "svm_fit": {"rows": int(len(Y)), "static": int(Y.sum()), "seconds": round(info["seconds"], 3),
                       "iterations": info["iterations"], "kkt_violation": info["violation"], "train_accuracy": round(acc, 4),
                       "support_vectors": int((info["alpha"] > 0).sum())}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
