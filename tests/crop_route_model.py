"""NumPy restatement of the DECISIONS of the crop kernels (3dal_pytorch_amd/csrc/dal3_crops.hip): which cell a
coordinate falls in, which cells a detection's ball marks, which lanes of which 64-point round hold members of which
detections, which of its three ways the fill pass takes for a round, and where every member's row lands in the flat
output. It is NOT a second implementation of the arithmetic: membership is handed in (oracle.ref_geom.points_in_rbbox
decides it), and a row's coordinates are judged against the exact rational value of the pose product (judge()).

The seams of the kernel are written in terms of the constants of the source, read from it here, so that the cases of
tests/crop_cases.py follow a change of CROP_CHUNK or CROP_WAVES.

TEST INFRASTRUCTURE ONLY: imported by tests/crop_cases.py, tests/test_crop_route_model.py (CPU) and
tests/test_gpu_crops_routes.py."""
import os
import re
from fractions import Fraction

import numpy as np

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dal_pytorch_amd", "csrc", "dal3_crops.hip")
_TEXT = open(_SRC).read()


def _const(name, pat=r"(\d+)"):
    return re.search(rf"^#define {name} {pat}", _TEXT, re.M).group(1)


CROP_CHUNK = int(_const("CROP_CHUNK"))                  # points per wavefront
CROP_WAVES = int(_const("CROP_WAVES"))                  # chunks per workgroup
CROP_GRID = int(_const("CROP_GRID"))                    # cells per side of the cull grid
CROP_CELL = np.float32(_const("CROP_CELL", r"([0-9.]+)f"))   # metres per cell
CROP_BATCH = int(_const("CROP_BATCH"))                  # detections per grid pass
ROUNDS = CROP_CHUNK // 64
assert CROP_BATCH == 64 and CROP_CHUNK % 64 == 0, "the model packs a batch's members into one 64-bit word per lane"

_F = np.float32


def cell(v):
    """crop_cell, operation by operation in float32: (v + GRID*CELL/2) * (1/CELL), clamped to [0, GRID-1] with
    fmaxf/fminf (a NaN gives 0), truncated."""
    v = np.asarray(v, _F)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v + _F(0.5) * _F(CROP_GRID) * CROP_CELL) * (_F(1.0) / CROP_CELL)
        t = np.fmin(np.fmax(t, _F(0.0)), _F(CROP_GRID - 1))
    return t.astype(np.int32)


def raster(spheres):
    """(K,4) float32 [cx,cy,cz,r^2] -> (K,4) int32 [cx0,cx1,cy0,cy1]: the inclusive rectangle of cells that the
    detection's bit is set in. The radius is rounded up (sqrtf, then 1.000001f); a non-finite radius or centre marks
    the whole grid."""
    sp = np.asarray(spheres, _F).reshape(-1, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        rad = np.sqrt(sp[:, 3]) * _F(1.000001)
        rect = np.stack([cell(sp[:, 0] - rad), cell(sp[:, 0] + rad), cell(sp[:, 1] - rad), cell(sp[:, 1] + rad)], 1)
    whole = ~(np.isfinite(rad) & np.isfinite(sp[:, 0]) & np.isfinite(sp[:, 1]))
    rect[whole] = [0, CROP_GRID - 1, 0, CROP_GRID - 1]
    return rect.astype(np.int32)


def n_chunks(n_pts):
    return (int(n_pts) + CROP_CHUNK - 1) // CROP_CHUNK


def rounds(points, inside, n_box):
    """One frame: points (P,3), inside (P,n_box) bool -> uint64 (chunks, batches, ROUNDS, 64): the member bitmask (bit j
    = detection batch*64 + j) that each lane holds in each round; lanes past the sweep's end hold 0."""
    p = int(np.asarray(points).shape[0])
    inside = np.asarray(inside, bool).reshape(p, n_box)
    nc, nb = n_chunks(p), (n_box + CROP_BATCH - 1) // CROP_BATCH
    pad = np.zeros((nc * CROP_CHUNK, nb * CROP_BATCH), bool)
    pad[:p, :n_box] = inside
    bits = pad.reshape(nc, ROUNDS, 64, nb, CROP_BATCH).transpose(0, 3, 1, 2, 4).astype(np.uint64)
    return (bits << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def route(masks):
    """The way crop_pass_kernel<true> takes for one round, from the 64 lanes' member masks:
    'empty'   no member lane (`__ballot(in != 0) == 0`)
    'single'  one member lane                                     } no lane differs from the first member lane's set:
    'run'     two or more member lanes, all holding the same set  } dup stays true, the ordered loop without the check
    'unique'  the sets differ, no detection has two members: one atomicAdd on s_row per member
    'ordered' the sets differ, some detection has two members: the ballot loop"""
    m = [int(x) for x in np.asarray(masks).reshape(64)]
    has = [x for x in m if x]
    if not has:
        return "empty"
    if all(x == has[0] for x in has):
        return "run" if len(has) > 1 else "single"
    seen = 0
    for x in has:                                    # s_seen: every member ORs its bits in and looks at what was there
        if seen & x:
            return "ordered"
        seen |= x
    return "unique"


def expected(points, inside, pose, order=None, capacity=None):
    """What a run must give. points / inside / pose: one frame's (P,3) float32, (P,K) bool and flat-16 pose, or lists of
    them (frames of one call; the detections are numbered frame by frame). order: output position -> detection;
    capacity: rows of the output buffer (None: as many as there are).
      counts   (K,)   members per detection
      start    (K+1,) rows in front of each detection, TRUE prefix sums in output order; [K] = total
      offsets  (K+1,) by output position, min(true, capacity)
      total, rows_written = min(total, capacity)
      index    per detection, the sweep indices of its members (increasing)
      det_frame (K,) frame of each detection
      src      (total,2) [frame, sweep index] of every row of the uncapped flat output; flat_index = src[:, 1]
      rows     (rows_written,3) float64: pose[:3] @ [x,y,z,1], NumPy's evaluation (judge() holds it and the device's
               to the exact value)"""
    if isinstance(points, np.ndarray):
        points, inside, pose = [points], [inside], [pose]
    index, det_frame = [], []
    for f, ins in enumerate(inside):
        ins = np.asarray(ins, bool)
        assert ins.ndim == 2 and ins.shape[0] == np.asarray(points[f]).shape[0]
        for k in range(ins.shape[1]):
            index.append(np.nonzero(ins[:, k])[0])
            det_frame.append(f)
    K = len(index)
    counts = np.array([len(i) for i in index], np.int64).reshape(K)
    order = np.arange(K) if order is None else np.asarray(order, np.int64)
    by_pos = np.concatenate([[0], np.cumsum(counts[order])]).astype(np.int64)
    start = np.empty(K + 1, np.int64)
    start[order] = by_pos[:-1]
    start[K] = total = int(by_pos[-1])
    cap = total if capacity is None else int(capacity)
    src = np.zeros((total, 2), np.int64)
    for k in range(K):
        src[start[k]:start[k] + counts[k], 0] = det_frame[k]
        src[start[k]:start[k] + counts[k], 1] = index[k]
    written = min(total, cap)
    rows = np.zeros((written, 3), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(len(points)):
            sel = np.nonzero(src[:written, 0] == f)[0]
            m = np.reshape(np.asarray(pose[f], np.float64), [4, 4])
            p = np.asarray(points[f], np.float32).astype(np.float64)[src[sel, 1]]
            rows[sel] = (m @ np.concatenate([p.T, np.ones((1, len(sel)))], 0))[:3].T
    return {"counts": counts, "start": start, "offsets": np.minimum(by_pos, cap), "total": total, "rows_written": written,
            "index": index, "det_frame": np.array(det_frame, np.int64), "src": src, "flat_index": src[:, 1].copy(),
            "rows": rows, "order": order, "capacity": cap}


def round_rows(exp, inside, chunk, rnd):
    """flat output rows of the members of one round of FRAME 0 -> {(detection, point): row}"""
    lo = chunk * CROP_CHUNK + rnd * 64
    out = {}
    for i in range(lo, min(lo + 64, inside.shape[0])):
        for k in np.nonzero(inside[i])[0]:
            out[(int(k), i)] = int(exp["start"][k] + np.searchsorted(exp["index"][k], i))
    return out


def exact_row(pose, xyz):
    """-> ([Fraction] * 3 exact value of pose[:3] @ [x,y,z,1], [Fraction] * 3 bound 5 * 2^-53 * sum |terms|): gamma_4, the
    forward error of a four-term double-precision dot product in any order, with or without FMA"""
    m = np.reshape(np.asarray(pose, np.float64), [4, 4])
    v = [Fraction(float(c)) for c in xyz] + [Fraction(1)]
    val, bound = [], []
    for i in range(3):
        terms = [Fraction(float(m[i, j])) * v[j] for j in range(4)]
        val.append(sum(terms))
        bound.append(Fraction(5, 2 ** 53) * sum(abs(t) for t in terms))
    return val, bound


def judge(got, exp, points, pose):
    """Hold one run's outputs against expected(): -> list of findings, empty when the run is right.
    got: 'counts' (K,), 'start' (K+1,), 'offsets' (K+1,), 'total', 'rows' (>= rows_written, 3) float64 and
    'flat_index' (>= rows_written,) — the flat buffers, of which the first rows_written rows are judged. points / pose:
    as handed to expected()."""
    if isinstance(points, np.ndarray):
        points, pose = [points], [pose]
    bad = []
    for name in ("counts", "start", "offsets"):
        if not np.array_equal(np.asarray(got[name]).reshape(-1), exp[name]):
            bad.append(f"{name}: got {np.asarray(got[name]).reshape(-1)[:12]}.., want {exp[name][:12]}..")
    if int(got["total"]) != exp["total"]:
        bad.append(f"total: got {got['total']}, want {exp['total']}")
    n = exp["rows_written"]
    rows, flat = np.asarray(got["rows"]), np.asarray(got["flat_index"]).reshape(-1)
    if rows.shape[0] < n or flat.shape[0] < n:
        return bad + [f"{rows.shape[0]} rows / {flat.shape[0]} indices, want {n}"]
    wrong = np.nonzero(flat[:n] != exp["flat_index"][:n])[0]
    if wrong.size:
        bad.append(f"index: {wrong.size} rows differ, first at row {wrong[0]}: got {flat[wrong[0]]}, want "
                   f"{exp['flat_index'][wrong[0]]}")
    # per detection: strictly increasing sweep indices, the members and nothing else (up to the cut)
    for k, want in enumerate(exp["index"]):
        lo = int(exp["start"][k])
        have = flat[min(lo, n):min(lo + len(want), n)]
        if have.size > 1 and not (np.diff(have) > 0).all():
            bad.append(f"detection {k}: indices not strictly increasing")
        if not np.array_equal(have, want[:have.size]):
            bad.append(f"detection {k}: indices {have[:8]}.. are not its members {want[:8]}..")
    # coordinates: within gamma_4 of the exact product; a NaN coordinate of the point gives a NaN row
    n_bad = 0
    for i in range(n):
        f, j = exp["src"][i]
        xyz = np.asarray(points[f], np.float32)[j]
        if not np.isfinite(xyz).all():
            ok = np.isnan(rows[i]).all() if np.isnan(xyz).any() else np.array_equal(rows[i], exp["rows"][i], equal_nan=True)
        else:
            val, bound = exact_row(pose[f], xyz)
            ok = bool(np.isfinite(rows[i]).all()) and all(abs(Fraction(float(rows[i, c])) - val[c]) <= bound[c]
                                                          for c in range(3))
        if not ok:
            n_bad += 1
            if n_bad <= 3:
                bad.append(f"row {i} (frame {f}, point {j}): got {rows[i]}, want {exp['rows'][i]}")
    if n_bad > 3:
        bad.append(f"... {n_bad} rows off in all")
    return bad
