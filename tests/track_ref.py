"""NumPy restatement of the tracking run (include/dal3.h, dal3_track / dal3_track_match): test infrastructure, the oracle
the kernels are held to, and the seeded inputs tests/golden/tracking.npz was recorded on.

track() restates PubTracker.step_centertrack (tools/waymo_tracking/tracker.py) over flat arrays — the same float32 /
float64 operations, the greedy assignment row by row — without the reference's per-detection dicts; match() restates
the `matching` loop of _create_pd_detection (waymo_common.py:173-189) with tests/iou_ref.py's IoU (float64) in place
of pcdet's boxes_iou3d_gpu.
"""
import numpy as np


def track(ct, tracking, label, score, frame_offsets, seq_offsets, max_age=3, max_dist=(0.8, 0.4, 0.6),
          score_thresh=0.75, id_base=0):
    """-> (per frame (box_ids, tracking_ids) int64 arrays, id_count)"""
    md = np.asarray(max_dist, np.float32)
    out, ids = [], int(id_base)
    starts = set(int(s) for s in seq_offsets[:-1])
    tr_ct = np.zeros((0, 2)); tr_tr = np.zeros((0, 2)); tr_lab = np.zeros(0, np.int32)
    tr_id = np.zeros(0, np.int64); tr_age = np.zeros(0, np.int64)
    for f in range(len(frame_offsets) - 1):
        if f in starts:
            tr_ct = tr_ct[:0]; tr_tr = tr_tr[:0]; tr_lab = tr_lab[:0]; tr_id = tr_id[:0]; tr_age = tr_age[:0]
        lo, hi = int(frame_offsets[f]), int(frame_offsets[f + 1])
        N, M = hi - lo, tr_ct.shape[0]
        if N == 0:
            tr_ct = tr_ct[:0]; tr_tr = tr_tr[:0]; tr_lab = tr_lab[:0]; tr_id = tr_id[:0]; tr_age = tr_age[:0]
            out.append((np.zeros(0, np.int64), np.zeros(0, np.int64)))
            continue
        c, t, lab, sc = ct[lo:hi], tracking[lo:hi], label[lo:hi], score[lo:hi]
        dets = (c + t.astype(np.float32)).astype(np.float32)
        col = np.full(N, -1, np.int64)
        if M > 0:
            tr32 = tr_ct.astype(np.float32)
            dist = np.sqrt(((tr32.reshape(1, -1, 2) - dets.reshape(-1, 1, 2)) ** 2).sum(axis=2))
            invalid = ((dist > md[lab].reshape(N, 1)) + (lab.reshape(N, 1) != tr_lab.reshape(1, M))) > 0
            dist = dist + invalid * 1e18
            for i in range(N):
                j = dist[i].argmin()
                if dist[i][j] < 1e16:
                    dist[:, j] = 1e18
                    col[i] = j
        matched = col >= 0
        fresh = ~matched & (sc.astype(np.float64) > score_thresh)
        taken = np.zeros(M, bool)
        taken[col[matched]] = True
        n_fresh = int(fresh.sum())
        new_ids = np.arange(ids + 1, ids + 1 + n_fresh)
        ids += n_fresh
        keep = ~taken & (tr_age < max_age)
        rows = np.concatenate([np.nonzero(matched)[0], np.nonzero(fresh)[0]])
        out_ids = np.concatenate([tr_id[col[matched]], new_ids]).astype(np.int64)
        out.append((rows.astype(np.int64), out_ids))
        tr_ct = np.concatenate([c[rows], tr_ct[keep] + tr_tr[keep] * -1])
        tr_tr = np.concatenate([t[rows], tr_tr[keep]])
        tr_lab = np.concatenate([lab[rows], tr_lab[keep]]).astype(np.int32)
        tr_id = np.concatenate([out_ids, tr_id[keep]])
        tr_age = np.concatenate([np.ones(len(rows), np.int64), tr_age[keep] + 1])
    return out, ids


def match(frames_out, boxes, frame_offsets, gt_boxes, gt_offsets, iou3d, thr=0.75):
    """-> per frame list of (frame, object index) or None, per output entry. iou3d(a (n,7), b (m,7)) -> (n,m). A
    non-finite box makes the row NaN: np.argmax takes the first NaN and NaN > thr fails (no match)."""
    matching, res = {}, []
    for f, (box_ids, tids) in enumerate(frames_out):
        g = gt_boxes[gt_offsets[f]:gt_offsets[f + 1]]
        row = []
        for k, tid in zip(box_ids, tids):
            tid = int(tid)
            if tid in matching:
                m = matching[tid]
            else:
                m = None
                if g.shape[0] > 0 and np.isfinite(boxes[frame_offsets[f] + k]).all() and np.isfinite(g).all():
                    iou = iou3d(boxes[frame_offsets[f] + k][None].astype(np.float64), g.astype(np.float64))[0]
                    b = int(np.argmax(iou))
                    if iou[b] > thr:
                        m = (f, b)
                        matching[tid] = m
            row.append(m)
        res.append(row)
    return res


# ---------------------------------------------------------------------------------------------- seeded inputs
def _pose(rng, identity=False):
    m = np.eye(4)
    if not identity:
        a = rng.uniform(-np.pi, np.pi)
        m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        m[:3, 3] = rng.uniform(-500, 500, 3)
    else:
        m[:3, 3] = [1000.0, -250.0, 3.0]
    return m.reshape(16)


def scene(seed, seqs=((3, 10), (7, 8), (12, 12)), n_obj=14, dt=0.1, identity_seq=1, clutter=4):
    """Frames of synthetic sequences in tracking order: per frame a dict token / frame_id / timestamp / box3d (K,9)
    float32 detector boxes [x,y,z,w,l,h,vx,vy,r] / label / score float32 / pose (flat-16) / gt (G,9) float32 annotation
    boxes / names. Objects move at constant velocity, so most detections match; the cases the tracker rules turn on
    are planted: an empty frame, exact distance ties (an identity-pose sequence), class mismatches, low scores,
    objects hidden longer than max_age, irregular time steps, a NaN translation, two detections on one track."""
    rng = np.random.default_rng(seed)
    frames = []
    for si, (seq_id, n_frames) in enumerate(seqs):
        ident = si == identity_seq
        pose = _pose(rng, ident)
        p0 = rng.uniform(-40, 40, (n_obj, 2))
        if ident:
            p0 = np.round(p0)
        vel = rng.uniform(-8, 8, (n_obj, 2)) * (0 if ident else 1)
        lab = rng.integers(0, 3, n_obj)
        size = rng.uniform(1, 5, (n_obj, 3))
        t = 0.0
        for fi in range(n_frames):
            if fi:
                t += dt * (1 + (fi % 3 == 2))                          # irregular time steps
            vis = np.ones(n_obj, bool)
            vis[2] = not (3 <= fi <= 7)                                # hidden longer than max_age
            vis[5] = fi % 2 == 0
            pos = p0 + vel * t
            rows = []
            for k in np.nonzero(vis)[0]:
                sc = np.float32(rng.uniform(0.3, 1.0)) if k % 4 == 0 else np.float32(rng.uniform(0.76, 1.0))
                rows.append([pos[k, 0], pos[k, 1], 0.5, size[k, 0], size[k, 1], size[k, 2], vel[k, 0], vel[k, 1],
                             rng.uniform(-3, 3), lab[k], sc])
            if ident:                                                  # a tie: tracks at x +- 1, a detection between
                if fi == 0:
                    rows += [[-60, 5, 0.5, 2, 4, 1.5, 0, 0, 0, 0, 0.9], [-59, 5, 0.5, 2, 4, 1.5, 0, 0, 0, 0, 0.9]]
                elif fi == 1:
                    rows += [[-59.5, 5, 0.5, 2, 4, 1.5, 0, 0, 0, 0, 0.9]]
                if fi == 2:                                            # class mismatch next to a track
                    rows += [[p0[0, 0] + 0.1, p0[0, 1], 0.5, 2, 4, 1.5, 0, 0, 0, (lab[0] + 1) % 3, 0.95]]
            if fi == 4 and si == 0:                                    # NaN translation
                rows += [[np.nan, 3.0, 0.5, 2, 4, 1.5, 0, 0, 0, 0, 0.9]]
            if fi == 5 and si == 2:                                    # two detections on one track
                rows += [[pos[1, 0] + 0.05, pos[1, 1], 0.5, 2, 4, 1.5, vel[1, 0], vel[1, 1], 0, lab[1], 0.9]]
            for _ in range(clutter):
                rows.append([*rng.uniform(-60, 60, 2), 0.5, 1, 1, 1, 0, 0, 0, rng.integers(0, 3), rng.uniform(0.2, 1.0)])
            if si == 2 and fi == 3:
                rows = []                                              # an empty frame
            rows = np.array(rows, np.float64).reshape(-1, 11)
            perm = rng.permutation(len(rows))
            rows = rows[perm]
            box3d = rows[:, :9].astype(np.float32)
            # detector convention: r2 = -r1 - pi/2 and (w, l): the reference's conversion undoes it
            gt = np.concatenate([box3d[:, :3], box3d[:, [4, 3, 5]], box3d[:, 6:8],
                                 (-box3d[:, 8:9] - np.pi / 2)], axis=1).astype(np.float32)
            jit = rng.uniform(-1, 1, gt.shape).astype(np.float32)
            gt[:, :2] += 0.35 * jit[:, :2] * np.minimum(gt[:, 3:5], 2)
            gt = gt[np.isfinite(gt).all(1)]
            keep_gt = rng.uniform(0, 1, len(gt)) > 0.2
            frames.append({"token": f"seq_{seq_id}_frame_{fi}.pkl", "frame_id": fi, "timestamp": 1.5e9 + t + seq_id * 100,
                           "box3d": box3d, "label": rows[:, 9].astype(np.int64), "score": rows[:, 10].astype(np.float32),
                           "pose": pose, "gt": gt[keep_gt], "names": [f"obj{seq_id}_{fi}_{g}" for g in range(int(keep_gt.sum()))]})
    return frames


def big_scene(seed, n_seq=300, n_frames=12, lo=20, hi=120, big_seq=0, big_n=700):
    """Larger seeded input straight in tracker form: (ct, tracking, label, score, frame_offsets, seq_offsets). One
    sequence holds > 500 live tracks."""
    rng = np.random.default_rng(seed)
    ct, tr, lab, sc, counts, starts = [], [], [], [], [], []
    for s in range(n_seq):
        starts.append(len(counts))
        n = big_n if s == big_seq else int(rng.integers(lo, hi))
        p = rng.uniform(-200, 200, (n, 2))
        v = rng.uniform(-1, 1, (n, 2))
        L = rng.integers(0, 3, n)
        for f in range(n_frames):
            vis = rng.uniform(0, 1, n) > 0.15
            if s % 17 == 5 and f == 6:
                vis[:] = False
            idx = np.nonzero(vis)[0]
            idx = idx[rng.permutation(len(idx))]
            lag = 0.0 if f == 0 else 0.1
            c = p[idx] + v[idx] * f * 0.1 + rng.normal(0, 0.05, (len(idx), 2))
            ct.append(c)
            tr.append(-v[idx] * lag)
            lab.append(L[idx])
            sc.append(rng.uniform(0.5, 1.0, len(idx)).astype(np.float32))
            counts.append(len(idx))
    fo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    so = np.asarray(starts + [len(counts)], np.int64)
    return (np.concatenate(ct), np.concatenate(tr), np.concatenate(lab).astype(np.int32), np.concatenate(sc), fo, so)
