"""NumPy restatement of the tracking run (include/dal3.h, dal3_track / dal3_track_match): test infrastructure, the oracle
the kernels are held to, and the seeded inputs tests/golden/tracking.npz was recorded on.

track() restates PubTracker.step_centertrack (tools/waymo_tracking/tracker.py) over flat arrays — the same float32 /
float64 operations, the greedy assignment row by row — without the reference's per-detection dicts; match() restates
the `matching` loop of _create_pd_detection (waymo_common.py:173-189) with tests/iou_ref.py's IoU (float64) in place
of pcdet's boxes_iou3d_gpu.
"""
import numpy as np


def track(ct, tracking, label, score, frame_offsets, seq_offsets, max_age=3, max_dist=(0.8, 0.4, 0.6),
          score_thresh=0.75, id_base=0, probe=None):
    """-> (per frame (box_ids, tracking_ids) int64 arrays, id_count). probe (stats() below): an object whose row() sees
    every row of the greedy loop and whose frame() sees every frame's sizes; it changes nothing."""
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
            dist0 = dist.copy() if probe is not None else None
            for i in range(N):
                j = dist[i].argmin()
                if probe is not None:
                    probe.row(f, i, dist0[i], dist[i])
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
        if probe is not None:
            probe.frame(f, N, M, int(matched.sum()), len(tr_id))
    return out, ids


def match(frames_out, boxes, frame_offsets, gt_boxes, gt_offsets, iou3d, thr=0.75):
    """-> per frame list of (frame, object index) or None, per output entry. iou3d(a (n,7), b (m,7)) -> (n,m). A
    non-finite box makes the row NaN: np.argmax takes the first NaN and NaN > thr fails (no match)."""
    matching, res = {}, []
    for f, (box_ids, tids) in enumerate(frames_out):
        g = gt_boxes[gt_offsets[f]:gt_offsets[f + 1]]
        row, iou_f = [], None                   # the frame's IoU matrix, computed once when a row first needs it
        for k, tid in zip(box_ids, tids):
            tid = int(tid)
            if tid in matching:
                m = matching[tid]
            else:
                m = None
                if g.shape[0] > 0 and np.isfinite(boxes[frame_offsets[f] + k]).all() and np.isfinite(g).all():
                    if iou_f is None:
                        iou_f = iou3d(boxes[frame_offsets[f]:frame_offsets[f + 1]].astype(np.float64), g.astype(np.float64))
                    iou = iou_f[k]
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


# ------------------------------------------------------------------ inputs for the paths the scenes above leave unrun
# All in tracker form (ct, tracking, label, score, frame_offsets, seq_offsets), like big_scene. stats() says what an
# input exercises, from the restatement's own loop.
class _Probe:
    def __init__(self):
        self.rows = self.rescanned = self.ties = self.matches = self.max_n = self.max_m = self.max_live = 0
        self.tie_sets = set()

    def row(self, f, i, before, now):
        """before: the row with no column taken (what the kernel's phase A sees); now: as greedy_assignment sees it"""
        self.rows += 1
        j0 = before.argmin()
        same = now[j0] == before[j0] or (np.isnan(now[j0]) and np.isnan(before[j0]))
        self.rescanned += not same
        tie = False
        for r in (before, now):
            m = r[r.argmin()]
            if m < 1e16:
                cols = np.nonzero(r == m)[0]
                if len(cols) > 1:
                    tie = True
                    self.tie_sets.add(tuple(int(c) for c in cols))
        self.ties += tie

    def frame(self, f, n, m, n_match, live):
        self.max_n, self.max_m, self.max_live = max(self.max_n, n), max(self.max_m, m), max(self.max_live, live)
        self.matches += n_match


def stats(ct, tracking, label, score, frame_offsets, seq_offsets, **params):
    """What the restatement's loop meets on an input: `rows` the detection rows with tracks present, `rescanned` those
    whose unconstrained argmin column (the first NaN column, if the row has one) an earlier row had taken, `ties` those
    whose minimum (below 1e16) is attained by more than one column, before or after the earlier rows' columns are
    removed, `tie_sets` the column sets of those minima, `max_n` / `max_m` the largest frame and track list met,
    `matches`, and `max_live` the longest track list after any frame. params as track()."""
    p = _Probe()
    with np.errstate(invalid="ignore"):
        track(ct, tracking, label, score, frame_offsets, seq_offsets, probe=p, **params)
    return {k: getattr(p, k) for k in ("rows", "rescanned", "ties", "max_n", "max_m", "matches", "max_live", "tie_sets")}


def _pack(frames, seq_starts):
    """frames: per frame (ct (n,2), tracking (n,2), label (n), score (n)); seq_starts: the first frame of each sequence
    (repeats allowed: a sequence without frames)"""
    ct = np.concatenate([np.asarray(f[0], np.float64).reshape(-1, 2) for f in frames] + [np.zeros((0, 2))])
    tr = np.concatenate([np.asarray(f[1], np.float64).reshape(-1, 2) for f in frames] + [np.zeros((0, 2))])
    lab = np.concatenate([np.asarray(f[2], np.int32).reshape(-1) for f in frames] + [np.zeros(0, np.int32)])
    sc = np.concatenate([np.asarray(f[3], np.float32).reshape(-1) for f in frames] + [np.zeros(0, np.float32)])
    fo = np.concatenate([[0], np.cumsum([len(np.asarray(f[2]).reshape(-1)) for f in frames])]).astype(np.int64)
    so = np.asarray(list(seq_starts) + [len(frames)], np.int64)
    return ct, tr, lab.astype(np.int32), sc.astype(np.float32), fo, so


def crowded_scene(seed, offset=0.0, continuous=False, seqs=((330, 8), (150, 6), (40, 5)), side=12, pitch=0.25):
    """Objects crowded far inside max_dist of one another: each sequence's objects sit on a side x side lattice of the
    given pitch (several per site), 85 % of them VEHICLE, and move by -1/8, 0 or 1/8 m per frame and axis; a detection
    is its object jittered by -1/8, 0 or 1/8 m. Everything is a multiple of 1/8 m, so the float32 distances are exact
    at the origin and with every coordinate shifted by offset = 300000.0 (float32 spacing 1/32 m) alike, and many are
    equal. 15-20 % of the objects are hidden per frame (tracks are kept and aged), the detections permuted per frame,
    scores 0.5..1. The first sequence's frames hold more than 256 detections and its track list passes 256, the
    second's passes 64. continuous=True: uniform positions, normal jitter (sigma 0.05 m) and velocities — no exact tie at
    the origin, ties by float32 rounding alone at 300000."""
    rng = np.random.default_rng(seed)
    frames, starts = [], []
    for n, n_frames in seqs:
        starts.append(len(frames))
        if continuous:
            p = rng.uniform(0, side * pitch, (n, 2))
            v = rng.normal(0, 0.05, (n, 2))
        else:
            p = rng.integers(0, side, (n, 2)) * pitch
            v = rng.integers(-1, 2, (n, 2)) * 0.125
        lab = np.where(rng.uniform(0, 1, n) < 0.85, 0, rng.integers(1, 3, n))
        for f in range(n_frames):
            hide = rng.permutation(n)[:int(n * rng.uniform(0.15, 0.20))]
            vis = np.ones(n, bool)
            vis[hide] = False
            idx = np.nonzero(vis)[0]
            idx = idx[rng.permutation(len(idx))]
            jit = rng.normal(0, 0.05, (len(idx), 2)) if continuous else rng.integers(-1, 2, (len(idx), 2)) * 0.125
            c = p[idx] + v[idx] * f + jit + offset
            frames.append((c, -v[idx] * (f > 0), lab[idx], rng.uniform(0.5, 1.0, len(idx)).astype(np.float32)))
    return _pack(frames, starts)


RING = np.array([(3, 4), (-3, -4), (4, 3), (-4, -3), (5, 0), (-5, 0), (0, 5), (0, -5), (-3, 4), (3, -4), (-4, 3),
                 (4, -3)], np.float64) / 8            # squared length 25/64, length 0.625: both exact in float32
TIE_RING_M = 130
TIE_RING_PAIRS = ((5, 69), (6, 69), (63, 64), (0, TIE_RING_M - 1), (31, 32))
# max_dist per class of tie_ring's variants: the ring distance itself (`dist > max_diff` is false: still a match) and the
# float32 just below it (nothing on a ring matches)
TIE_RING_MAX_DIST = {"default": (0.8, 0.4, 0.6), "exact": (0.625, 0.4, 0.6),
                     "below": (float(np.nextafter(np.float32(0.625), np.float32(0))), 0.4, 0.6)}
TIE_RING_MANY = (10, 20, 33, 40, 62, 65, 70, 95, 96, 100, 127, 128)      # the columns of the ring with 12 tracks


def tie_ring():
    """Exact ties at chosen columns. Frame 0 has TIE_RING_M detections of high score and no tracks, so column k of
    frame 1's track list is row k (id k + 1). VEHICLE tracks sit on circles of radius 0.625 (RING) around centres far
    apart; a frame-1 detection at a centre is equidistant from its ring. The tied columns are TIE_RING_PAIRS —
    {5, 69} one lane of the wave on two strides, {6, 69} the higher lane holding the lower column (the row sits
    0.625 from both and farther from 5), {63, 64} across the wave's stride, {0, M - 1}, {31, 32} across a word of
    the taken bitmap, that ring at 3e5 m — and the twelve columns of TIE_RING_MANY on one ring. Several rows sit at one
    centre: each later one must take the next-lowest free column on a re-scan, and those past the ring's size match
    nothing. Every other column is a PEDESTRIAN track, some exactly at the centres (distance 0, another class).
    Frame 2 repeats frame 0's positions: the ids show which track every row took."""
    M = TIE_RING_M
    a, c, d, e, g = (np.array(x, np.float64) for x in ((10, 10), (40, -20), (-30, 50), (3e5, -3e5), (80, 80)))
    b = a + RING[0] - RING[2]                  # 0.625 from column 69 (a + RING[0]); sqrt(29)/8 from column 5
    pos = np.zeros((M, 2))
    lab = np.ones(M, np.int32)
    ring_cols = {5: a + RING[1], 69: a + RING[0], 6: b + RING[5], 63: c + RING[4], 64: c + RING[7], 0: d + RING[8],
                 M - 1: d + RING[3], 31: e + RING[6], 32: e + RING[9]}
    for k, col in enumerate(TIE_RING_MANY):
        ring_cols[col] = g + RING[k]
    fill = [j for j in range(M) if j not in ring_cols]
    for n, j in enumerate(fill):
        pos[j] = (a, c, d, e, g)[n] if n < 5 else (-200.0 - 3 * n, 7.0)
    for j, p in ring_cols.items():
        pos[j], lab[j] = p, 0
    rows = [a, b, a, a, c, c, c, d, e, e, d, d] + [g] * 14
    f1 = np.array(rows)
    zero = lambda n: np.zeros((n, 2))          # noqa: E731
    frames = [(pos, zero(M), lab, np.full(M, 0.9, np.float32)),
              (f1, zero(len(f1)), np.zeros(len(f1), np.int32), np.full(len(f1), 0.9, np.float32)),
              (pos, zero(M), lab, np.full(M, 0.5, np.float32))]
    return _pack(frames, [0])


def nonfinite_scene():
    """NaN and inf positions and a NaN score, max_age 3 (the comments say what each must do). VEHICLE throughout, nothing
    moves, objects 10 m apart.
    Sequence 0 — f0: 8 tracks (columns 0..7). f1: rows at tracks 0..3 take columns 0..3; then a NaN row: its first NaN
    column, 0, is taken, the next free one, 4, decides: no match; it scores 0.9, so it becomes a NaN track; a second NaN
    row (NaN y) likewise; the row after them, at track 5, still matches (the NaN tracks are not in this frame's list).
    f2-f4: two NaN tracks live: every row's argmin is the first NaN column, so nothing matches — rows of score 0.9
    get new ids every frame, rows of score 0.5 get none. f5: the NaN tracks are gone after max_age frames unmatched, the
    rows match again, the lowest column of the equal tracks born in f2-f4.
    Sequence 1 — f0: 5 tracks and a +inf detection, which becomes an inf track. f1: a +inf row is NaN at that column
    only (inf - inf) and infinitely far from the rest: no match, a second inf track; a (-inf, 0) row is inf from
    everything: no match; the finite rows after them match as if neither were there; one unmatched row has a NaN score:
    not fresh. f2: the same finite rows match again."""
    V = lambda n: np.zeros(n, np.int32)        # noqa: E731
    Z = lambda n: np.zeros((n, 2))             # noqa: E731
    hi, lo, nan, inf = np.float32(0.9), np.float32(0.5), np.nan, np.inf
    p = np.stack([np.arange(8) * 10.0, np.zeros(8)], axis=1)
    frames = [(p, Z(8), V(8), np.full(8, hi))]
    f1 = np.concatenate([p[:4] + 0.125, [[nan, 3.0]], [[55.0, nan]], p[5:6] + 0.125])
    frames.append((f1, Z(7), V(7), np.full(7, hi)))
    for _ in range(3):
        frames.append((np.concatenate([p[:3] + 0.25, p[5:8]]), Z(6), V(6), np.array([hi] * 3 + [lo] * 3)))
    frames.append((np.concatenate([p[:3] + 0.25, p[5:8]]), Z(6), V(6), np.full(6, hi)))
    frames.append((np.concatenate([p[:3] + 0.25, p[5:8]]), Z(6), V(6), np.full(6, hi)))
    s1 = len(frames)
    q = np.stack([np.arange(5) * 10.0, np.full(5, 100.0)], axis=1)
    frames.append((np.concatenate([q, [[inf, 100.0]]]), Z(6), V(6), np.full(6, hi)))
    f1 = np.concatenate([q[:1], [[inf, 100.0]], [[-inf, 0.0]], q[1:] + 0.125, [[500.0, 500.0]]])
    frames.append((f1, Z(8), V(8), np.array([hi] * 7 + [nan], np.float32)))
    frames.append((q, Z(5), V(5), np.full(5, hi)))
    return _pack(frames, [0, s1])


THRESHOLD_SCORES = (np.float32(0.75), np.nextafter(np.float32(0.75), np.float32(1)), np.float32(0.6))
THRESHOLD_HIDDEN = (0, 1, 2, 3, 4)


def threshold_scene():
    """The score threshold and max_age at their edges. Rows 0..2 of every frame are three objects that score
    THRESHOLD_SCORES — exactly float32(0.75): not above score_thresh 0.75, never a track; the next float32: a track;
    float32(0.6) = 0.60000002...: above 0.6 in the reference's float64 comparison though equal in float32, so a track at
    score_thresh 0.6 — rows never matched before they become tracks. Then five objects of score 0.9, object h hidden for
    the h frames after frame 0 (THRESHOLD_HIDDEN): its track, age 1 at frame 0, is kept while age < max_age, so it
    survives iff h < max_age — for max_age 0..3 that is hidden max_age - 1 (kept), max_age and max_age + 1 (a new id) —
    and two objects always seen. Nothing moves; objects 10 m apart."""
    n_frames = 7
    frames = []
    for f in range(n_frames):
        pos, sc = [(0.0, k * 10.0) for k in range(3)], list(THRESHOLD_SCORES)
        for h in THRESHOLD_HIDDEN:
            if f == 0 or f > h:
                pos.append((100.0 + 10 * h, 0.0))
                sc.append(np.float32(0.9))
        pos += [(300.0, 0.0), (310.0, 0.0)]
        sc += [np.float32(0.9)] * 2
        n = len(pos)
        frames.append((np.array(pos), np.zeros((n, 2)), np.zeros(n, np.int32), np.array(sc, np.float32)))
    return _pack(frames, [0])


EDGE_NM = tuple((n, m) for n in (255, 256, 257) for m in (31, 32, 33, 63, 64, 65, 255, 256, 257))


def _pair_frames(n, m, rng):
    """frame 0: m detections of score 0.9 on a line 1/2 m apart, the class by position; frame 1: n detections, row i at
    track (7 i) mod m shifted by a multiple of 1/16 m — with n > m several rows per track, a re-scan for most"""
    pos = np.stack([np.arange(m) * 0.5, np.zeros(m)], axis=1)
    lab = (np.arange(m) // 5) % 3
    at = (7 * np.arange(n)) % m
    c = pos[at] + rng.integers(-2, 3, (n, 2)) / 16
    return [(pos, np.zeros((m, 2)), lab, np.full(m, 0.9, np.float32)),
            (c, np.zeros((n, 2)), lab[at], rng.uniform(0.5, 1.0, n).astype(np.float32))]


def edge_layouts():
    """{name: inputs} of small structural cases: no sequence; frames without a detection; sequences without a frame
    (repeated seq_offsets entries) first, in the middle and last; a sequence whose first frame is empty; one whose
    frames are all empty; a single detection; and `pairs`: one two-frame sequence for each (N, M) of EDGE_NM — frame 0
    leaves M tracks, frame 1 has N detections near them."""
    rng = np.random.default_rng(7)
    one = lambda x, s=0.9: (np.array([[x, 0.0]]), np.zeros((1, 2)), [0], [s])      # noqa: E731
    two = lambda x: (np.array([[x, 0.0], [x + 5, 0.0]]), np.zeros((2, 2)), [0, 1], [0.9, 0.8])   # noqa: E731
    none = (np.zeros((0, 2)), np.zeros((0, 2)), [], [])
    out = {"S0": _pack([], []), "K0": _pack([none, none, none], [0, 2]),
           "no_frames": _pack([two(0), two(0.1), one(3), two(3.1)], [0, 0, 2, 2, 4]),
           "first_empty": _pack([two(0), two(0.1), none, two(0.2), two(0.3), one(9)], [0, 2, 5]),
           "all_empty": _pack([two(0), two(0.1), none, none, two(0.2), two(0.3)], [0, 2, 4]),
           "single": _pack([one(1.5)], [0])}
    frames, starts = [], []
    for n, m in EDGE_NM:
        starts.append(len(frames))
        frames += _pair_frames(n, m, rng)
    out["pairs"] = _pack(frames, starts)
    return out


def many_frames(n_seq=33000, seed=3):
    """n_seq sequences of two frames with one or two detections each: more frames than the match kernels' grid cap of
    65,535 and more sequences than one block of the id scan. Frame 1's detections sit 1/8 m from frame 0's (a match
    where both exist) or 50 m away (a new id); a quarter of the scores are below the threshold."""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 3, (n_seq, 2))                     # detections of (sequence, frame)
    counts = n.reshape(-1)
    fo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    K = int(fo[-1])
    frame = np.repeat(np.arange(2 * n_seq), counts)
    k_in = np.arange(K) - fo[frame]                        # 0 or 1: which detection of its frame
    far = rng.uniform(0, 1, K) < 0.2
    ct = np.stack([k_in * 10.0 + (frame % 2) * 0.125 + far * (frame % 2) * 50.0, (frame // 2) % 97 * 1.0], axis=1)
    lab = (rng.integers(0, 3, n_seq)[frame // 2]).astype(np.int32)
    sc = np.where(rng.uniform(0, 1, K) < 0.25, 0.5, 0.9).astype(np.float32)
    return ct, np.zeros((K, 2)), lab, sc, fo, np.arange(0, 2 * n_seq + 1, 2).astype(np.int64)


def dense_cases():
    """{name: (inputs, track() parameters)}: every seeded input above with the parameters it is meant for, the cases
    tests/golden/tracking_dense.npz records the reference's tracker on (many_frames is left out there)."""
    out = {"crowded": (crowded_scene(21), {}), "crowded_far": (crowded_scene(21, offset=300000.0), {}),
           "continuous": (crowded_scene(22, continuous=True), {}),
           "continuous_far": (crowded_scene(22, offset=300000.0, continuous=True), {})}
    for k, md in TIE_RING_MAX_DIST.items():
        out["tie_ring_" + k] = (tie_ring(), {"max_dist": md})
    out["nonfinite"] = (nonfinite_scene(), {})
    for ma in (0, 1, 2, 3):
        out[f"threshold_age{ma}"] = (threshold_scene(), {"max_age": ma})
    out["threshold_0.6"] = (threshold_scene(), {"score_thresh": 0.6})
    for k, v in edge_layouts().items():
        out["edge_" + k] = (v, {})
    return out
