#!/usr/bin/env python3
"""The tracking run at the size of a Waymo split: ~200 sequences x 198 frames x 100-300 detections (objects at
consistent velocities, so most detections match). Times, on the current GPU:
  tracker   dal3_track alone (CUDA events, median of --reps)
  match     dal3_track_match alone, against per-frame annotation boxes near the detections
  call      track_sequences + frames(): upload of the flat inputs, the kernel, the per-frame download
  oracle    the NumPy restatement (tests/track_ref.py) on --oracle_seqs sequences, scaled to the split (host)
and checks the kernel's ids against the restatement on those sequences. One JSON line; --out writes it to a file.
    python tools/bench_track.py [--seqs 200 --frames 198 --reps 5 --out profiles/bench_track.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
trk = importlib.import_module("3dal_pytorch_amd.track")
import track_ref  # noqa: E402


def split_input(seed, S, F):
    """flat tracker inputs: per sequence n ~ U[100, 300] objects, each visible in ~90 % of the frames"""
    rng = np.random.default_rng(seed)
    ct, tr, lab, sc, counts = [], [], [], [], []
    starts = []
    for s in range(S):
        starts.append(len(counts))
        n = int(rng.integers(100, 301))
        p, v, L = rng.uniform(-75, 75, (n, 2)), rng.uniform(-10, 10, (n, 2)), rng.integers(0, 3, n)
        for f in range(F):
            idx = np.nonzero(rng.uniform(0, 1, n) > 0.1)[0]
            idx = idx[rng.permutation(len(idx))]
            ct.append(p[idx] + v[idx] * 0.1 * f + rng.normal(0, 0.03, (len(idx), 2)))
            tr.append(-v[idx] * (0.0 if f == 0 else 0.1))
            lab.append(L[idx])
            sc.append(rng.uniform(0.3, 1.0, len(idx)).astype(np.float32))
            counts.append(len(idx))
    fo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return (np.concatenate(ct), np.concatenate(tr), np.concatenate(lab).astype(np.int32), np.concatenate(sc), fo,
            np.asarray(starts + [len(counts)], np.int64))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), [round(t, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=200)
    ap.add_argument("--frames", type=int, default=198)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle_seqs", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    ct, tr, lab, sc, fo, so = split_input(7, a.seqs, a.frames)
    K = len(lab)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d = dict(seq_offsets=t(so), frame_offsets=t(fo), ct=t(ct), tracking=t(tr), label=t(lab), score=t(sc))
    b = trk.TrackInputs.__new__(trk.TrackInputs)
    b.counts, b.seq_offsets = np.diff(fo), so
    cap = b.capacity(3)
    res = trk.track_sequences(**d, capacity=cap)                      # warm-up
    torch.cuda.synchronize()
    t_track, all_track = timed(lambda: trk.track_sequences(**d, capacity=cap), a.reps)
    res = trk.track_sequences(**d, capacity=cap)
    frames = res.frames()
    boxes = np.zeros((K, 7), np.float32)
    boxes[:, :2], boxes[:, 3:6] = ct, (4.5, 2.0, 1.6)
    gt = boxes.copy()
    gt[:, :2] += np.random.default_rng(1).normal(0, 0.2, (K, 2))
    db, dg, dgo = t(boxes), t(gt), t(fo)
    trk.match_ground_truth(res, db, dgo, dg)
    t_match, all_match = timed(lambda: trk.match_ground_truth(res, db, dgo, dg), a.reps)
    mf, _ = trk.match_ground_truth(res, db, dgo, dg)
    n_matched = int((mf >= 0).sum().item())

    def call():
        dd = dict(seq_offsets=t(so), frame_offsets=t(fo), ct=t(ct), tracking=t(tr), label=t(lab), score=t(sc))
        trk.track_sequences(**dd, capacity=cap).frames()
    call()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        call()
    t_call = (time.perf_counter() - t0) / a.reps * 1e3
    # the restated CPU tracker on the first sequences, and the ids it gives
    q = a.oracle_seqs
    f_end = int(so[q])
    t0 = time.perf_counter()
    want, _ = track_ref.track(ct[:fo[f_end]], tr[:fo[f_end]], lab[:fo[f_end]], sc[:fo[f_end]], fo[:f_end + 1], so[:q + 1])
    t_oracle = (time.perf_counter() - t0) * 1e3
    ok = all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(frames[:f_end], want))
    n_out = int(sum(len(x[0]) for x in frames))
    rec = {"bench": "track", "device": torch.cuda.get_device_name(0), "sequences": a.seqs, "frames": int(len(fo) - 1),
           "detections": K, "capacity": cap, "outputs": n_out, "ids": res.total(), "match_share": round(n_out and
           (n_out - 0) / K, 4), "gt_matched": n_matched,
           "tracker_ms": round(t_track, 3), "tracker_ms_all": all_track, "match_ms": round(t_match, 3),
           "match_ms_all": all_match, "track_call_ms": round(t_call, 2),
           "oracle_ms_per_sequence": round(t_oracle / q, 1), "oracle_ms_split_estimate": round(t_oracle / q * a.seqs, 0),
           "oracle_equal_on_first_sequences": bool(ok), "reps": a.reps}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
