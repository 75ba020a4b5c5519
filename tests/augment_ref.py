"""The training input restated in NumPy (3dal_pytorch_amd/augment.py; dal3_gt_paste_select, dal3_augment_points and
dal3_augment_boxes of include/dal3.h), the seeded inputs of tests/golden/gen_augment.py, and the measures the tests judge by.

Every function takes `dt`: numpy.float32 restates the kernels (one rounding per operation, sin and cos of an angle formed in
float64 and rounded once), numpy.float64 is the truth the rotation is judged against. tests/golden/gen_augment.py asserts
the restatement against the reference's own functions; tests/test_augment_cpu.py asserts it against the archive.

`fault=` plants one wrong reading at a time: no_clear (a rejected candidate's row and column stay live), no_containment
(the two containment loops skipped), vel_not_flipped, vel_not_scaled, unstable_rank (equal order keys in reverse source
order)."""
import os
import pickle

import numpy as np

F32, F64 = np.float32, np.float64
FAULTS = ("no_clear", "no_containment", "vel_not_flipped", "vel_not_scaled", "unstable_rank")
CLASS_NAMES = ["VEHICLE", "PEDESTRIAN", "CYCLIST"]
TASKS = [dict(num_class=1, class_names=["VEHICLE"]), dict(num_class=2, class_names=["PEDESTRIAN", "CYCLIST"])]
GROUPS = [{"VEHICLE": 6}, {"PEDESTRIAN": 4}, {"CYCLIST": 3}]
PC_RANGE = [-20.0, -16.0, -3.0, 20.0, 16.0, 3.0]
VOXEL = [0.5, 0.5, 0.15]
MAX_OBJS = 40
SIZES = {"VEHICLE": (2.0, 4.5, 1.6), "PEDESTRIAN": (0.8, 0.9, 1.7), "CYCLIST": (0.8, 1.8, 1.6), "SIGN": (0.3, 0.3, 2.0),
         "UNKNOWN": (1.0, 1.0, 1.0)}
DB_COUNTS = {"VEHICLE": 9, "PEDESTRIAN": 7, "CYCLIST": 5}
DB_PREP = [dict(filter_by_min_num_points=dict(VEHICLE=5, PEDESTRIAN=2, CYCLIST=2)), dict(filter_by_difficulty=[-1])]

# The GPU test's bar for the rotated columns, a multiple of the yardstick (the reference's own float32 output against its
# float64 output, from the archive), by the rule written beside pillars_ref.BARS: the worst ratio of the first MI355X run
# x at most 2, one significant digit, under a tenth of the smallest planted-fault ratio of tests/test_augment_cpu.py
# (1e3); a bar comes down or stays, it does not go up. Before that run it stood at 4 on reasoning: kernel and yardstick
# are float32 evaluations of the same two-term dot product followed by two roundings (scale, translation); they differ in
# the last bit of the rounded sine and cosine and in whether the products are fused, each at most one more rounding of a
# term. The first run (profiles/augment_measured.json, DAL3_AUGMENT_RECORD over tests/test_gpu_augment.py: the four rotated
# samples of the batches) recorded at worst 1.478 for the points (B/s3) and 1.000 for the boxes: x 2 gives 2.96 -> 3.
BAR = 3.0


def class_id(name):
    return CLASS_NAMES.index(name) + 1 if name in CLASS_NAMES else (-1 if name in ("DontCare", "ignore", "UNKNOWN") else 0)


# ------------------------------------------------------------------------------------------------ inputs
def _boxes(rs, names, spread=14.0, speed=3.0):
    out = np.zeros((len(names), 9), F32)
    for i, n in enumerate(names):
        w, l, h = SIZES[n]
        out[i] = [rs.uniform(-spread, spread), rs.uniform(-spread * 0.8, spread * 0.8), rs.uniform(-1, 1), w * rs.uniform(0.9, 1.1),
                  l * rs.uniform(0.9, 1.1), h, rs.uniform(-speed, speed), rs.uniform(-speed, speed), rs.uniform(-3.1, 3.1)]
    return out


def database(F, seed=7):
    """-> (infos: class name -> list of the reference's entries, clouds: path -> (n, F) float32). Objects of 1 .. 200 points;
    the first of each class fails filter_by_min_num_points, the second filter_by_difficulty."""
    rs = np.random.RandomState(seed + F)
    infos, clouds = {}, {}
    for name, count in DB_COUNTS.items():
        boxes = _boxes(rs, [name] * count)
        infos[name] = []
        for i in range(count):
            n = 1 if i == 0 else int(rs.randint(5, 201))
            path = f"db/{name}_{i}.bin"
            clouds[path] = (rs.standard_normal((n, F)) * 0.4).astype(F32)
            infos[name].append(dict(name=name, path=path, box3d_lidar=boxes[i], num_points_in_gt=n, difficulty=-1 if i == 1 else 0,
                                    image_idx=i, gt_idx=i))
    return infos, clouds


def write_database(root, infos, clouds):
    os.makedirs(os.path.join(root, "db"), exist_ok=True)
    for path, pts in clouds.items():
        pts.tofile(os.path.join(root, path))
    with open(os.path.join(root, "dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f)
    return os.path.join(root, "dbinfos.pkl")


def kept_objects(infos):
    """the database after DB_PREP, flattened in class order -> [(name, entry)]"""
    out = []
    for name, objs in infos.items():
        need = DB_PREP[0]["filter_by_min_num_points"][name]
        out += [(name, o) for o in objs if o["num_points_in_gt"] >= need and o["difficulty"] not in DB_PREP[1]["filter_by_difficulty"]]
    return out


SAMPLES = {
    # name: F, scene points, GT names, rotation noise, translate std, shuffle, sampler, no_augmentation, seed
    "s0": dict(F=5, n=3000, names=["VEHICLE", "VEHICLE", "PEDESTRIAN", "CYCLIST", "SIGN", "UNKNOWN", "VEHICLE"], rot=0.78539816, std=0, seed=11),
    "s1": dict(F=5, n=65, names=["VEHICLE", "PEDESTRIAN", "CYCLIST"], rot=[0, 0], std=0.5, seed=12),
    "s2": dict(F=5, n=1, names=[], rot=0.78539816, std=0, seed=13),
    "s3": dict(F=5, n=63, names=["PEDESTRIAN"] * 5 + ["VEHICLE"], rot=0.78539816, std=[0.2, 0.3, 0.1], seed=14),
    "s4": dict(F=4, n=64, names=["VEHICLE", "CYCLIST"], rot=[0, 0], std=0, seed=15),
    "s5": dict(F=5, n=0, names=["VEHICLE", "PEDESTRIAN"], rot=0.78539816, std=0, seed=16, sampler=False),
    "s6": dict(F=5, n=64, names=["VEHICLE", "SIGN", "CYCLIST"], rot=0.78539816, std=0, seed=17, no_augmentation=True),
    "s7": dict(F=5, n=64, names=["PEDESTRIAN", "VEHICLE"], rot=[0, 0], std=0, seed=18, shuffle=False),
}
BATCHES = {"A": ["s0", "s1"], "B": ["s2", "s3", "s5"], "C": ["s4"], "D": ["s6"], "E": ["s7"]}
SCALE_NOISE = [0.95, 1.05]


def sample_inputs(name):
    """-> scene (n, F) float32, gt_boxes (g, 9) float32, gt_names"""
    s = SAMPLES[name]
    rs = np.random.RandomState(1000 + s["seed"])
    scene = np.concatenate([rs.uniform(-22, 22, (s["n"], 2)), rs.uniform(-3, 3, (s["n"], 1)), rs.uniform(0, 1, (s["n"], s["F"] - 3))], 1).astype(F32)
    boxes = _boxes(rs, s["names"])
    if name == "s0":
        boxes[0, :2], boxes[0, 8] = [-24.0, -4.0], 0.3     # one corner inside the range after the sample's transform
        boxes[1, :2] = [27.0, -21.0]                        # wholly outside it
        boxes[2, 8] = 3.1                                   # its angle crosses pi under the transforms
    return scene, boxes, list(s["names"])


def collision_cases():
    """hand-made layouts at the thresholds, all axis-aligned with dyadic coordinates, so that float32 evaluates every
    quantity exactly: [(tag, gt boxes, [(class name, candidate box)])]. The expected flags are the reference's."""
    def box(x, y, w, l):
        return [x, y, 0.0, w, l, 1.5, 0.0, 0.0, 0.0]
    V, P, C = "VEHICLE", "PEDESTRIAN", "CYCLIST"
    return [
        ("touching", [box(0, 0, 2, 2)], [(V, box(2, 0, 2, 2)), (V, box(0, -2, 2, 2))]),
        ("identical", [box(0, 0, 2, 4)], [(V, box(0, 0, 2, 4)), (V, box(8, 0, 2, 4)), (V, box(8, 0, 2, 4))]),
        ("inside", [box(0, 0, 8, 8)], [(V, box(0.5, 0.5, 1, 1))]),
        ("contains", [box(0, 0, 1, 1)], [(V, box(0.5, 0.25, 8, 8))]),
        ("zero_width", [box(0, 0, 4, 4)], [(V, box(0, 0, 0, 8)), (V, box(1, 0, 0, 1)), (V, box(10, 0, 0, 2))]),
        ("chain", [], [(V, box(0, 0, 2, 2)), (V, box(1.5, 0.5, 2, 2)), (V, box(3, 1, 2, 2))]),
        # A accepted; B collides with A and is rejected; C collides only with B and is accepted
        ("chain_classes", [], [(V, box(0, 0, 2, 2)), (P, box(1.5, 0.5, 2, 2)), (P, box(3, 1, 2, 2))]),
        ("forward", [], [(P, box(0, 0, 2, 2)), (P, box(1, 1, 2, 2))]),
        ("later_class", [box(20, 20, 1, 1)], [(V, box(0, 0, 4, 4)), (P, box(1, 1, 1, 1)), (P, box(6, 0, 1, 1)), (C, box(6.5, 0.25, 1, 1))]),
        ("no_gt_no_hit", [], [(C, box(0, 0, 1, 1))]),
    ]


# ------------------------------------------------------------------------------------------------ the paste
def corners(boxes, dt=F32):
    """center_to_corner_box2d(boxes[:, :2], boxes[:, 3:5], boxes[:, 8]) -> (n, 4, 2)"""
    b = np.asarray(boxes).reshape(-1, 9).astype(dt)
    sn, cs = np.sin(b[:, 8].astype(F64)).astype(dt), np.cos(b[:, 8].astype(F64)).astype(dt)
    out = np.zeros((b.shape[0], 4, 2), dt)
    for k, (nx, ny) in enumerate(((-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5))):
        px, py = b[:, 3] * dt(nx), b[:, 4] * dt(ny)
        out[:, k, 0] = (px * cs + py * sn) + b[:, 0]
        out[:, k, 1] = (px * -sn + py * cs) + b[:, 1]
    return out


def collide(a, q, fault=None, trace=None):
    """box_collision_test's entry for corners a (4, 2) against q (4, 2), in their dtype. trace gets (difference, scale) of
    every comparison taken."""
    def cmp(lhs, rhs, strict=True):
        if trace is not None:
            trace.append((float(lhs) - float(rhs), abs(float(lhs)) + abs(float(rhs))))
        return lhs > rhs if strict else lhs >= rhs
    zero = a.dtype.type(0)
    for ax in (0, 1):
        if not cmp(min(a[:, ax].max(), q[:, ax].max()) - max(a[:, ax].min(), q[:, ax].min()), zero):
            return False
    for k in range(4):
        A, B = a[k], a[(k + 1) % 4]
        for l in range(4):
            C, D = q[l], q[(l + 1) % 4]
            acd = cmp((D[1] - A[1]) * (C[0] - A[0]), (C[1] - A[1]) * (D[0] - A[0]))
            bcd = cmp((D[1] - B[1]) * (C[0] - B[0]), (C[1] - B[1]) * (D[0] - B[0]))
            if acd != bcd:
                abc = cmp((C[1] - A[1]) * (B[0] - A[0]), (B[1] - A[1]) * (C[0] - A[0]))
                abd = cmp((D[1] - A[1]) * (B[0] - A[0]), (B[1] - A[1]) * (D[0] - A[0]))
                if abc != abd:
                    return True
    if fault == "no_containment":
        return False

    def inside(out, inn):
        for l in range(4):
            for k in range(4):
                vec = -(out[k] - out[(k + 1) % 4])
                if cmp(vec[1] * (out[k, 0] - inn[l, 0]), vec[0] * (out[k, 1] - inn[l, 1]), strict=False):
                    return False
        return True
    return inside(a, q) or inside(q, a)


def collision_matrix(gt_boxes, cand_boxes, dt=F32, fault=None, traces=None):
    """-> (nc, ng + nc) bool: candidate i against the GT boxes, then the candidates; the diagonal false"""
    gt_boxes, cand_boxes = np.asarray(gt_boxes, F32).reshape(-1, 9), np.asarray(cand_boxes, F32).reshape(-1, 9)
    c = corners(np.concatenate([gt_boxes, cand_boxes]), dt)
    ng, nc = len(gt_boxes), len(cand_boxes)
    m = np.zeros((nc, ng + nc), bool)
    for i in range(nc):
        for j in range(ng + nc):
            if j != ng + i:
                t = None if traces is None else []
                m[i, j] = collide(c[ng + i], c[j], fault, t)
                if traces is not None:
                    traces[(i, j)] = t
    return m


def accept(coll, ng, groups, fault=None):
    """sample_class_v2's serial loop over the groups of sample_all -> (nc) bool"""
    nc = len(groups)
    ok, rejected = np.zeros(nc, bool), np.zeros(nc, bool)
    for i in range(nc):
        hit = False
        for j in range(ng + nc):
            live = True
            if j >= ng:
                c = j - ng
                live = ok[c] if groups[c] < groups[i] else (fault == "no_clear" or not rejected[c]) if groups[c] == groups[i] else False
            hit |= bool(live and coll[i, j] and j != ng + i)
        rejected[i], ok[i] = hit, not hit
    return ok


# ------------------------------------------------------------------------------------------------ the points
def points(scene, cand_rows, cand_boxes, ok, xform, keys, dt=F32, transform=True, fault=None):
    """scene (n, F), cand_rows: the candidates' (r, F) arrays, xform (7): flip y, flip x, rotation, scale, translation;
    keys: one per source row (the candidates' rows first) or None -> (rows, F); a rejected candidate's rows are NaN"""
    parts, valid = [], []
    for r, box, a in zip(cand_rows, cand_boxes, ok):
        p = np.asarray(r, F32).copy()
        p[:, :3] += np.asarray(box, F32)[:3]              # the reference moves the object's float32 rows in place: one float32 rounding
        parts.append(p.astype(dt))
        valid.append(np.full(len(p), bool(a)))
    parts.append(np.asarray(scene, F32).astype(dt))
    valid.append(np.ones(len(scene), bool))
    src, valid = np.concatenate(parts), np.concatenate(valid)
    if transform:
        if xform[0]:
            src[:, 1] = -src[:, 1]
        if xform[1]:
            src[:, 0] = -src[:, 0]
        sn, cs = dt(np.sin(F64(xform[2]))), dt(np.cos(F64(xform[2])))
        x, y = src[:, 0].copy(), src[:, 1].copy()
        src[:, 0], src[:, 1] = x * cs + y * sn, x * -sn + y * cs
        src[:, :3] *= dt(xform[3])
        src[:, :3] = (src[:, :3].astype(F64) + np.asarray(xform[4:7], F64)).astype(dt)
    src[~valid] = np.nan
    if keys is None:
        return src
    keys = np.asarray(keys, np.int64)
    order = np.lexsort((-np.arange(len(keys)), keys)) if fault == "unstable_rank" else np.argsort(keys, kind="stable")
    return src[order]


# ------------------------------------------------------------------------------------------------ the boxes
def in_range(c, bv_range, dt=F32):
    """filter_gt_box_outside_range's test for corners (n, 4, 2): any corner strictly inside minmax_to_corner_2d's polygon"""
    r = np.asarray(bv_range, F32).astype(dt)
    d = r[2:] - r[:2]
    poly = np.array([[d[0] * dt(0) + r[0], d[1] * dt(0) + r[1]], [d[0] * dt(0) + r[0], d[1] + r[1]], [d[0] + r[0], d[1] + r[1]],
                     [d[0] + r[0], d[1] * dt(0) + r[1]]], dt)
    keep = np.zeros(len(c), bool)
    margins = []
    for i in range(len(c)):
        for p in c[i]:
            inside = True
            for k in range(4):
                vec = poly[k] - poly[k - 1]
                cross = vec[1] * (poly[k, 0] - p[0]) - vec[0] * (poly[k, 1] - p[1])
                margins.append((float(cross), abs(float(vec[1] * poly[k, 0])) + abs(float(vec[1] * p[0])) + abs(float(vec[0] * poly[k, 1])) + abs(float(vec[0] * p[1]))))
                if cross >= 0:
                    inside = False
                    break
            keep[i] |= inside
    return keep, margins


def boxes(gt_boxes, gt_cls, cand_boxes, cand_cls, ok, xform, pc_range=PC_RANGE, n_classes=3, max_objs=MAX_OBJS, dt=F32,
          transform=True, fault=None, margins=None):
    """-> (gt_boxes_and_cls (max_objs, 10), count, overflow)"""
    gt_boxes, cand_boxes = np.asarray(gt_boxes, F32).reshape(-1, 9), np.asarray(cand_boxes, F32).reshape(-1, 9)
    b = np.concatenate([gt_boxes, cand_boxes]).astype(dt)
    cls = np.concatenate([np.asarray(gt_cls, np.int64).reshape(-1), np.asarray(cand_cls, np.int64).reshape(-1)])
    keep = (cls >= 1) & (cls <= n_classes) & np.concatenate([np.ones(len(gt_boxes), bool), np.asarray(ok, bool).reshape(-1)])
    if transform:
        pi, two_pi = dt(np.pi), dt(2 * np.pi)
        if xform[0]:
            b[:, 1], b[:, 8] = -b[:, 1], -b[:, 8] + pi
            if fault != "vel_not_flipped":
                b[:, 7] = -b[:, 7]
        if xform[1]:
            b[:, 0], b[:, 8] = -b[:, 0], -b[:, 8] + two_pi
            if fault != "vel_not_flipped":
                b[:, 6] = -b[:, 6]
        ang = F64(xform[2])
        sn, cs = dt(np.sin(ang)), dt(np.cos(ang))
        x, y = b[:, 0].copy(), b[:, 1].copy()
        b[:, 0], b[:, 1] = x * cs + y * sn, x * -sn + y * cs
        vx, vy = b[:, 6].astype(F64), b[:, 7].astype(F64)
        b[:, 6], b[:, 7] = (vx * np.cos(ang) + vy * np.sin(ang)).astype(dt), (vx * -np.sin(ang) + vy * np.cos(ang)).astype(dt)
        b[:, 8] += dt(xform[2])
        b[:, :6 if fault == "vel_not_scaled" else 8] *= dt(xform[3])
        b[:, :3] = (b[:, :3].astype(F64) + np.asarray(xform[4:7], F64)).astype(dt)
    r = np.asarray(pc_range, F32)
    inside, m = in_range(corners(b, dt), r[[0, 1, 3, 4]], dt)
    if margins is not None:
        margins += m
    keep &= inside
    period = dt(2 * np.pi)
    b[:, 8] = b[:, 8] - np.floor(b[:, 8] / period + dt(0.5)) * period
    rows = [np.concatenate([b[i, [0, 1, 2, 3, 4, 5, 8, 6, 7]], [dt(c)]]) for c in range(1, n_classes + 1) for i in np.nonzero(keep & (cls == c))[0]]
    out = np.zeros((max_objs, 10), dt)
    n = min(len(rows), max_objs)
    if n:
        out[:n] = np.stack(rows)[:n]
    return out, n, len(rows) > max_objs


# ------------------------------------------------------------------------------------------------ the measures
def column_ratio(got, f32, truth):
    """per column: max |got - truth| over max |f32 - truth| (the reference's own float32 error), the largest over the columns
    whose yardstick is not zero; a column the reference gets exactly must be exact here too -> (ratio, exact_ok)"""
    got, f32, truth = (np.asarray(v, F64) for v in (got, f32, truth))
    if not truth.size:
        return 0.0, True
    e, y = np.abs(got - truth).max(0), np.abs(f32 - truth).max(0)
    live = y > 0
    return (float((e[live] / y[live]).max()) if live.any() else 0.0), bool(np.all(e[~live] == 0))
