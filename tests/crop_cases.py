"""Planted scenes for the crop kernels (3dal_pytorch_amd/csrc/dal3_crops.hip), shared by tests/test_crop_route_model.py
(CPU: does every case hit what it claims?) and tests/test_gpu_crops_routes.py (does the device give what the model
expects?).

A case is built from a pool: boxes on a 5 m lattice inside +-30 m (l in [2,4], w in [2,2.6]: the circumscribed circles
of neighbours never meet), nested boxes sharing a lattice site where a case wants a point inside two or three
detections, and float32 points drawn in and around the boxes. oracle.ref_geom.points_in_rbbox says which detections
each pool point belongs to; the sweep is then assembled lane by lane from pool points with the wanted sets. The
oracle alone decides membership, the layout decides the route.

get(name) -> dict: 'sweeps' [(P,3) float32], 'dets' [(K,9) float32, the detector's convention], 'poses' [flat 16], and
what the case claims to hit:
  'routes'  [(frame, chunk, batch, round, route)]      crop_route_model.route of that round
  'members' [(frame, point, detection of the frame)]   planted members (seams)
  'skips'   [(frame, chunk, batch)]                    a batch without a member in a chunk that has members of others
  'all_member' [(frame, point)]                        NaN points: members of every detection
  'some' / 'none' [(frame, detection)]                 detections that must have / must not have members
truth(name) -> the oracle's (P,K) membership per frame."""
import functools

import numpy as np

import crop_route_model as M
from _common import synth
from oracle import ref_geom as G

CHUNK, WAVES = M.CROP_CHUNK, M.CROP_WAVES
_SITES = np.array([(x, y) for y in range(-30, 31, 5) for x in range(-30, 31, 5)], np.float64)
_f32 = np.float32


def inside_of(points, box9):
    if box9.shape[0] == 0:
        return np.zeros((points.shape[0], 0), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        return G.points_in_rbbox(points, G.waymo_boxes(box9))


class Scene:
    """n_box lattice boxes (detector convention) and the pool to draw points with a wanted membership set from. nests:
    tuples of detection indices (outer, inner, innermost) that share the outer one's site and yaw, each 0.6 of the
    one around it."""

    def __init__(self, seed, n_box, nests=()):
        rng = self.rng = np.random.default_rng(seed)
        site = _SITES[rng.permutation(len(_SITES))[:n_box]]
        b = np.zeros((n_box, 9))
        b[:, :2] = site
        b[:, 2] = rng.uniform(-0.2, 0.2, n_box)
        b[:, 3] = rng.uniform(2.0, 2.6, n_box)                    # w
        b[:, 4] = rng.uniform(2.0, 4.0, n_box)                    # l
        b[:, 5] = rng.uniform(1.5, 2.0, n_box)
        b[:, 6:8] = rng.normal(0.0, 1.0, (n_box, 2))
        b[:, 8] = rng.uniform(-np.pi, np.pi, n_box)
        for nest in nests:
            for level, k in enumerate(nest[1:], 1):
                b[k] = b[nest[0]]
                b[k, 3:6] *= 0.6 ** level
        self.box9 = b.astype(_f32)
        self.K = n_box

    def pick(self, dets, n):
        """n float32 points whose membership set, by the oracle, is exactly `dets` (() = no detection)"""
        dets = tuple(sorted(dets))
        if n == 0 or self.K == 0:
            dets = ()
        rng, got, have = self.rng, [], 0
        want = np.zeros(self.K, bool)
        want[list(dets)] = True
        for _ in range(200):
            m = 4 * n + 32 if dets else n + n // 8 + 32
            if dets:
                k = min(dets, key=lambda d: float(self.box9[d, 3]) * float(self.box9[d, 4]))
                rad = 0.45 * float(self.box9[k, 3:5].min()) * np.sqrt(rng.uniform(0, 1, m))
                ang = rng.uniform(0, 2 * np.pi, m)
                xy = self.box9[k, :2].astype(np.float64) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
                z = float(self.box9[k, 2]) + rng.uniform(-0.4, 0.4, m) * float(self.box9[k, 5])
            else:                                                 # between four lattice sites
                xy = _SITES[rng.integers(0, len(_SITES), m)] + 2.5 + rng.uniform(-0.1, 0.1, (m, 2))
                z = rng.uniform(-1.0, 1.0, m)
            cand = np.concatenate([xy, z[:, None]], 1).astype(_f32)
            good = cand[(inside_of(cand, self.box9) == want).all(1)] if self.K else cand
            got.append(good[:n - have])
            have += got[-1].shape[0]
            if have >= n:
                return np.concatenate(got)
        raise AssertionError(f"the pool has no {n} points of set {dets}")

    def points_for(self, sets):
        """one point per entry of `sets` (tuples of detections), in that order"""
        sets = [tuple(sorted(s)) for s in sets]
        out = np.zeros((len(sets), 3), _f32)
        for s in set(sets):
            where = [i for i, t in enumerate(sets) if t == s]
            out[where] = self.pick(s, len(where))
        return out

    def sweep(self, n, planted):
        """n points, none in a detection, except planted {position: set}"""
        sets = [()] * n
        for i, s in planted.items():
            sets[i] = s
        return self.points_for(sets)


def _case(name, sweeps, dets, **claims):
    poses = [synth.pose_veh_to_global(77, f"{name}{f}") for f in range(len(sweeps))]
    out = {"name": name, "sweeps": [np.ascontiguousarray(s, _f32).reshape(-1, 3) for s in sweeps],
           "dets": [np.ascontiguousarray(d, _f32).reshape(-1, 9) for d in dets], "poses": poses}
    for key in ("routes", "members", "skips", "all_member", "some", "none"):
        out[key] = claims.pop(key, [])
    out.update(claims)
    return out


def _round(lanes):
    """{lane: set} -> 64 sets"""
    return [lanes.get(i, ()) for i in range(64)]


# ---------------------------------------------------------------------------------------------------------- routes
def _run_one_box():
    sc = Scene(1, 5)
    sets = [()] * 128 + [(2,)] * 64 + [()] * 10                   # round 2 of chunk 0: 64 consecutive points of box 2
    return _case("run_one_box", [sc.points_for(sets)], [sc.box9], routes=[(0, 0, 0, 2, "run")])


def _run_pair(a, b):
    sc = Scene(10 + a, 64, nests=((a, b),))
    sets = [()] * CHUNK
    sets[17] = (a, b)                                             # the pair's rows in chunk 1 do not start at 0
    sets += [()] * 64 + _round({i: (a, b) for i in range(64) if i % 8 < 5}) + [()] * 3
    return _case(f"run_pair_{a}_{b}", [sc.points_for(sets)], [sc.box9], routes=[(0, 1, 0, 1, "run")])


def _unique(n):
    sc = Scene(20 + n, 130)
    dets = [10, 45] if n == 2 else list(sc.rng.permutation(n))
    lanes = sc.rng.permutation(64)[:n]
    sets = [()] * 64 + _round({int(l): (int(d),) for l, d in zip(lanes, dets)}) + [()] * 30
    return _case(f"unique_{n}", [sc.points_for(sets)], [sc.box9], routes=[(0, 0, 0, 1, "unique")])


_NEST3 = (5, 20, 45)


def _unique_nested():
    sc = Scene(30, 64, nests=(_NEST3,))
    others = [k for k in range(64) if k not in _NEST3]
    lanes = [i for i in range(64) if i != 17]
    rnd = {17: _NEST3}
    rnd.update({l: (k,) for l, k in zip(lanes, sc.rng.permutation(others))})
    sets = _round(rnd) + [()] * 5
    return _case("unique_nested", [sc.points_for(sets)], [sc.box9], routes=[(0, 0, 0, 0, "unique")])


def _ordered_interleaved():
    sc = Scene(31, 64)
    sets = [()] * 64 + [(7,) if i % 2 == 0 else (50,) for i in range(64)] + [()] * 9
    return _case("ordered_interleaved", [sc.points_for(sets)], [sc.box9], routes=[(0, 0, 0, 1, "ordered")])


def _ordered_nested():
    sc = Scene(32, 64, nests=(_NEST3,))
    others = [k for k in range(64) if k not in _NEST3][:30]
    rnd = {3: (5,), 10: _NEST3, 40: (5, 20)}
    rnd.update({12 + i: (k,) for i, k in enumerate(others) if 12 + i != 40})
    sets = _round(rnd) + [()] * 20
    return _case("ordered_nested", [sc.points_for(sets)], [sc.box9], routes=[(0, 0, 0, 0, "ordered")])


_PAIR = (9, 47)
_CARRIED = ("unique", "ordered", "run", "unique")


def _carried_rounds():
    """four rounds that take unique, ordered, run, unique for detections 2, 33 and the nested pair (9, 47)"""
    r0 = _round({5: (2,), 20: (33,), 41: _PAIR})
    r1 = {i: ((2,) if i % 2 == 0 else (33,)) for i in range(20)}
    r1.update({30: _PAIR, 31: (9,)})
    r2 = _round({i: _PAIR for i in range(10, 30)})
    r3 = _round({1: (33,), 2: _PAIR, 63: (2,)})
    return r0 + _round(r1) + r2 + r3


def _carried():
    sc = Scene(33, 64, nests=(_PAIR,))
    first = [()] * CHUNK
    first[7], first[100], first[CHUNK - 1] = (2,), _PAIR, (33,)
    sets = first + _carried_rounds() + [()] * 37
    return _case("carried", [sc.points_for(sets)], [sc.box9], routes=[(0, 1, 0, r, w) for r, w in enumerate(_CARRIED)])


def _batch_skip():
    sc = Scene(34, 140)
    sets = [()] * CHUNK + [()] * 100
    sets[3], sets[64], sets[500] = (3,), (135,), (3,)             # chunk 0: batches 0 and 2
    sets[CHUNK + 9], sets[CHUNK + 70] = (70,), (70,)              # chunk 1: batch 1 only
    return _case("batch_skip", [sc.points_for(sets)], [sc.box9], skips=[(0, 0, 1), (0, 1, 0), (0, 1, 2)])


# ----------------------------------------------------------------------------------------------------------- seams
SIZES = [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, WAVES * CHUNK - 1, WAVES * CHUNK, WAVES * CHUNK + 1,
         (WAVES + 1) * CHUNK + 1]


def _seam_frame(seed, n):
    """first and last point, the last lane of the first round, both sides of every chunk (and so workgroup) boundary"""
    sc = Scene(seed, 3)
    spots = sorted({0, n - 1, 63} | {c * CHUNK - d for c in range(1, n // CHUNK + 2) for d in (0, 1)})
    spots = [i for i in spots if 0 <= i < n]
    planted = {i: (j % 3,) for j, i in enumerate(spots)}
    return sc.sweep(n, planted), sc.box9, [(i, s[0]) for i, s in planted.items()]


def _seam_points(n):
    pts, box9, mem = _seam_frame(40, n)
    return _case(f"seam_points_{n}", [pts], [box9], members=[(0, i, k) for i, k in mem])


def _seam_ragged():
    frames = [_seam_frame(41 + f, n) for f, n in enumerate(SIZES)]
    return _case("seam_ragged", [f[0] for f in frames], [f[1] for f in frames],
                 members=[(f, i, k) for f, fr in enumerate(frames) for i, k in fr[2]])


def _seam_scan():
    """a second trip of the scan's 64-chunk loop: members in chunks 62, 63 and 64 of a 65-chunk frame; a short frame
    beside it"""
    sc = Scene(60, 2)
    n = 64 * CHUNK + 1
    planted = {62 * CHUNK + 5: (0,), 63 * CHUNK - 1: (1,), 63 * CHUNK: (0,), 63 * CHUNK + 700: (0,), 64 * CHUNK - 1: (1,),
               64 * CHUNK: (1,), 3: (1,)}
    small = Scene(61, 2)
    return _case("seam_scan", [sc.sweep(n, planted), small.sweep(70, {69: (1,)})], [sc.box9, small.box9],
                 members=[(0, i, s[0]) for i, s in planted.items()] + [(1, 69, 1)])


DET_COUNTS = [0, 1, 63, 64, 65, 127, 128, 129]


def _det_frame(seed, k):
    """members in detections 0, 31, 32 and 63 of the first and of the last batch"""
    sc = Scene(seed, k)
    last = ((k - 1) // M.CROP_BATCH) * M.CROP_BATCH if k else 0
    dets = sorted({b + j for b in (0, last) for j in (0, 31, 32, 63) if b + j < k})
    n = CHUNK + 70
    planted = {}
    for j, d in enumerate(dets):
        for i in (11 + j, 64 * (j + 2) + 63 - j, CHUNK - 1 - j, CHUNK + 2 * j):
            planted[i] = (d,)
    return sc.sweep(n, planted), sc.box9, [(i, s[0]) for i, s in planted.items()]


def _det_count(k):
    pts, box9, mem = _det_frame(70, k)
    return _case(f"det_count_{k}", [pts], [box9], members=[(0, i, d) for i, d in mem])


def _det_ragged():
    frames = [_det_frame(71 + f, k) for f, k in enumerate(DET_COUNTS)]
    return _case("det_ragged", [f[0] for f in frames], [f[1] for f in frames],
                 members=[(f, i, d) for f, fr in enumerate(frames) for i, d in fr[2]])


# ------------------------------------------------------------------------------------------------------ non-finite
def _nonfinite_points(k):
    sc = Scene(80 + k, k)
    n = 200
    planted = {5: (0,), 63: (k - 1,), 64: (31,), 130: (k - 1,), 131: (0,), 150: (64,)}
    pts = sc.sweep(n, planted)
    nan, inf = np.nan, np.inf
    pts[0, 0] = nan                                               # NaN in x only
    pts[70, 2] = nan                                              # NaN in z only
    pts[100, 0] = inf
    pts[101, 0] = -inf
    pts[199] = [nan, nan, nan]
    return _case(f"nonfinite_points_{k}", [pts], [sc.box9], all_member=[(0, 0), (0, 70), (0, 199)], infinite=[(0, 100), (0, 101)],
                 members=[(0, i, s[0]) for i, s in planted.items()])


def _nonfinite_boxes():
    sc = Scene(85, 6)
    planted = {3: (0,), 64: (1,), 65: (3,), 200: (5,), 299: (0,)}
    pts = sc.sweep(300, planted)
    box9 = sc.box9.copy()
    box9[2, 0] = np.nan                                           # a NaN centre
    box9[4, 4] = np.inf                                           # an infinite length
    return _case("nonfinite_boxes", [pts], [box9], members=[(0, i, s[0]) for i, s in planted.items()])


# ------------------------------------------------------------------------------------------------------- cull grid
def _box9(cx, cy, cz, l, w, h, yaw):
    """Waymo-convention numbers -> a detector row (crops.waymo_boxes turns it back)"""
    return [cx, cy, cz, w, l, h, 0.0, 0.0, -yaw - np.pi / 2]


def _around(rng, box9, n):
    """n points per box in its circumscribed circle (in and out), plus its centre"""
    out = []
    for b in np.asarray(box9, np.float64):
        r = 0.55 * np.hypot(b[3], b[4]) * np.sqrt(rng.uniform(0, 1, n))
        a = rng.uniform(0, 2 * np.pi, n)
        out.append(np.stack([b[0] + r * np.cos(a), b[1] + r * np.sin(a), b[2] + rng.uniform(-0.6, 0.6, n) * b[5]], 1))
        out.append(b[None, :3])
    return np.concatenate(out).astype(_f32)


def _steps(v):
    v = _f32(v)
    return [np.nextafter(v, _f32(-np.inf)), v, np.nextafter(v, _f32(np.inf))]


def _cull_borders():
    c = float(M.CROP_CELL)
    edge = 0.5 * M.CROP_GRID * c                                  # 75 m
    up, dn = (lambda v: float(np.nextafter(_f32(v), _f32(np.inf)))), (lambda v: float(np.nextafter(_f32(v), _f32(-np.inf))))
    box9 = np.array([_box9(2 * c, 4 * c, 0.0, 3.0, 3.0, 2.0, 0.4),            # 0: centred on a cell corner
                     _box9(up(3 * c), dn(-5 * c), 0.1, 3.0, 2.5, 2.0, -1.0),  # 1, 2: one float32 step off cell borders
                     _box9(dn(-8 * c), up(9 * c), -0.1, 3.0, 2.5, 2.0, 2.5),
                     _box9(edge - 0.5, 20.0, 0.0, 4.0, 2.0, 2.0, 0.2),        # 3, 4, 5: straddling the grid's edges
                     _box9(-edge - 0.2, -20.1, 0.0, 4.0, 2.0, 2.0, 2.0),
                     _box9(12.0, -edge + 0.1, 0.0, 4.0, 2.0, 2.0, 1.3),
                     _box9(edge + 15.0, edge + 20.0, 0.0, 4.0, 2.0, 2.0, 1.0),  # 6: wholly beyond
                     _box9(-40.0, 40.0, 0.5, 20.0, 8.0, 3.0, 0.7),             # 7: 20 m, many cells
                     _box9(30.0, -30.0, 0.0, 0.0, 2.0, 2.0, 0.3)], _f32)       # 8: zero length
    rng = np.random.default_rng(90)
    pts = [_around(rng, box9, 40)]
    for k in (0, 1, 2):                                           # on the cell borders next to the centre, and a step either side
        cx, cy = (round(float(v) / c) * c for v in box9[k, :2])
        pts.append(np.array([[x, y, 0.0] for x in _steps(cx) for y in _steps(cy)], _f32))
    pts.append(np.array([[x, 20.0, 0.0] for x in _steps(edge)] + [[x, -20.1, 0.0] for x in _steps(-edge)]
                        + [[12.0, y, 0.0] for y in _steps(-edge)], _f32))
    pts = np.concatenate(pts)
    pts = pts[rng.permutation(pts.shape[0])]
    return _case("cull_borders", [pts], [box9], some=[(0, k) for k in range(8)], none=[(0, 8)])


def _cull_whole_grid():
    box9 = np.array([_box9(0.0, 0.0, 0.0, 250.0, 250.0, 10.0, 0.3), _box9(10.0, 10.0, 0.0, 3.0, 2.0, 2.0, 0.5),
                     _box9(-20.0, 5.0, 0.0, 3.0, 2.0, 2.0, -0.5)], _f32)
    rng = np.random.default_rng(91)
    far = np.stack([rng.uniform(-90, 90, 80), rng.uniform(-90, 90, 80), rng.uniform(-6, 6, 80)], 1).astype(_f32)
    pts = np.concatenate([far, _around(rng, box9[1:], 30)])
    return _case("cull_whole_grid", [pts[rng.permutation(pts.shape[0])]], [box9], some=[(0, 0), (0, 1), (0, 2)])


def _cull_far():
    box9 = np.array([_box9(1.0e4, -1.0e4, 1.0, 4.0, 2.0, 2.0, 0.5), _box9(1.0e4 + 6.0, -1.0e4, 1.0, 3.0, 2.0, 2.0, -0.9)], _f32)
    rng = np.random.default_rng(92)
    return _case("cull_far", [_around(rng, box9, 150)], [box9], some=[(0, 0), (0, 1)])


# ------------------------------------------------------------------------------------------- faces of rotated boxes
def _nudge(v, s):
    for _ in range(abs(s)):
        v = np.nextafter(_f32(v), _f32(np.inf if s > 0 else -np.inf))
    return _f32(v)


def _faces():
    """points on the six faces of three rotated boxes, each moved by -2..+2 float32 steps in x, in y, in z and in all
    three: the fp32 evaluation order of the face equations decides which side they fall on"""
    box9 = np.array([_box9(10.0, 5.0, 0.5, 4.0, 2.0, 1.5, 0.3), _box9(-17.3, 22.1, -0.4, 3.3, 1.9, 1.7, 1.1),
                     _box9(33.7, -41.2, 1.0, 2.5, 2.2, 1.6, -2.2)], _f32)
    corners = G.box_corners(G.waymo_boxes(box9)).astype(np.float64)
    pts = []
    for k in range(3):
        for face in G._FACE:
            p0, p1, p2 = corners[k, face]
            for u, v in ((0.3, 0.6), (0.7, 0.25)):
                base = (p1 + u * (p0 - p1) + v * (p2 - p1)).astype(_f32)
                for s in range(-2, 3):
                    for axes in ((0,), (1,), (2,), (0, 1, 2)):
                        q = base.copy()
                        for a in axes:
                            q[a] = _nudge(q[a], s)
                        pts.append(q)
    return _case("faces", [np.array(pts, _f32)], [box9], both_outcomes=True)


# ------------------------------------------------------------------------------------------ capacity, order, reuse
def _capacity():
    """three frames of the same 64 tracked objects, laid out track-major; frame 0's rounds 0 and 1 take the unique and
    the ordered route (where the capacities of the test cut)"""
    sweeps, dets = [], []
    for f in range(3):
        sc = Scene(100 + f, 64, nests=(_PAIR,))
        sweeps.append(sc.points_for(_carried_rounds() + [()] * (40 + f)))
        dets.append(sc.box9)
    order = np.array([f * 64 + k for k in range(64) for f in range(3)], np.int64)
    return _case("capacity", sweeps, dets, order=order,
                 routes=[(f, 0, 0, r, w) for f in range(3) for r, w in enumerate(_CARRIED)])


def _reuse():
    """the same plan on points A, then on points B: as many, other members; detections 2 and 33 lose theirs, 50 gains"""
    sc = Scene(110, 64, nests=(_PAIR,))
    sets_a = [()] * 30 + _carried_rounds() + [()] * (CHUNK - 200)
    sets_b = [((50,) if s in ((2,), (33,)) else s) for s in reversed(sets_a)]
    sets_b[0], sets_b[CHUNK // 2] = (12,), _PAIR
    return _case("reuse", [sc.points_for(sets_a)], [sc.box9], sweeps_b=[sc.points_for(sets_b)], emptied=[2, 33])


_BUILD = {"run_one_box": _run_one_box, "unique_nested": _unique_nested, "ordered_interleaved": _ordered_interleaved,
          "ordered_nested": _ordered_nested, "carried": _carried, "batch_skip": _batch_skip, "seam_ragged": _seam_ragged,
          "seam_scan": _seam_scan, "det_ragged": _det_ragged, "nonfinite_boxes": _nonfinite_boxes,
          "cull_borders": _cull_borders, "cull_whole_grid": _cull_whole_grid, "cull_far": _cull_far, "faces": _faces,
          "capacity": _capacity, "reuse": _reuse}
for _a, _b in ((3, 40), (31, 32), (62, 63)):
    _BUILD[f"run_pair_{_a}_{_b}"] = functools.partial(_run_pair, _a, _b)
for _n in (2, 33, 64):
    _BUILD[f"unique_{_n}"] = functools.partial(_unique, _n)
for _n in SIZES:
    _BUILD[f"seam_points_{_n}"] = functools.partial(_seam_points, _n)
for _k in DET_COUNTS:
    _BUILD[f"det_count_{_k}"] = functools.partial(_det_count, _k)
for _k in (65, 129):
    _BUILD[f"nonfinite_points_{_k}"] = functools.partial(_nonfinite_points, _k)

NAMES = sorted(_BUILD)
ROUTE_CASES = [n for n in NAMES if n.startswith(("run_", "unique_", "ordered_", "carried", "batch_skip"))]
CULL_CASES = [n for n in NAMES if n.startswith("cull_")]


@functools.lru_cache(maxsize=None)
def get(name):
    return _BUILD[name]()


@functools.lru_cache(maxsize=None)
def truth(name):
    c = get(name)
    return [inside_of(p, d) for p, d in zip(c["sweeps"], c["dets"])]
