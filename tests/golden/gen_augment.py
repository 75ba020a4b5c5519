#!/usr/bin/env python3
"""Generate tests/golden/augment.npz from the REAL reference (jacky121298/3DAL_PyTorch): its own `Preprocess.__call__`
(det3d/datasets/pipelines/preprocess.py, train mode), `DataBaseSamplerV2.sample_all` (det3d/core/sampler/sample_ops.py)
over a small synthetic database written to a temporary directory, `filter_gt_box_outside_range` and `box_collision_test`
(det3d/core/sampler/preprocess.py) and `AssignLabel.__call__`, on the seeded inputs of tests/augment_ref.py.

Run only where the reference checkout exists (DAL3_REFERENCE, as tests/golden/gen_pillars.py reads it):
    python tests/golden/gen_augment.py

The files are loaded by path behind gen_center_loss.py's stubs (numba's decorators as identity, the registries). One thing
numba does and plain Python does not is put right: `box_collision_test` asks `ret[i, j] is True` / `is False` of a
boolean array element, which numba compiles as equality and CPython evaluates as the identity of a numpy.bool_ with a
singleton, never true, so that the containment loops would never run. The module's text is therefore executed with
` is True` / ` is False` read as ` == True` / ` == False`, which is what the reference computes under numba.

What is recorded, per sample of augment_ref.SAMPLES: the candidates the sampler offered (indices into the filtered database)
and their groups, the pair matrix of the reference's `box_collision_test` over the GT boxes and all candidates, the accepted
flags, the draws the reference made (np.random.choice, uniform, normal and shuffle are wrapped; the shuffle is stored as order
keys over this project's source rows, a valid row's key being its output position), the points out and gt_boxes_and_cls,
each also from float64 copies of the inputs under the same draws (stored as the float32 output plus a float32 difference).
For augment_ref.collision_cases: the pair matrix and the flags. For the sampler alone: the candidate lists of a sequence of
calls that runs through a reset.

Asserted here: the restatement of tests/augment_ref.py against all of it, and that no discrete decision (a stand-up overlap,
an orientation product, a containment cross product, a corner against the range) sits within 1e-4 relative of its
threshold unless float32 evaluates it exactly. A pair or box that does would be excluded and listed; the cap is 0. Fixed
timestamps: a rerun reproduces the archive byte for byte."""
import copy
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gen_center_loss as GC  # noqa: E402
import gen_pillars as G  # noqa: E402
import gen_roi as GR  # noqa: E402
import augment_ref as A  # noqa: E402

MARGIN = 1e-4
MAX_EXCLUDED = 0


class Cfg(dict):
    __getattr__ = dict.__getitem__


class Log:
    @staticmethod
    def info(*a):
        pass


def import_reference():
    pre, _, _ = GC.import_reference()
    G._stub("det3d.utils")
    G._stub("det3d.utils.check", shape_mergeable=lambda x, shape: True)
    path = os.path.join(G.REF, "det3d/core/sampler/preprocess.py")
    text = open(path).read().replace(" is True", " == True").replace(" is False", " == False")
    prep = types.ModuleType("det3d.core.sampler.preprocess")
    sys.modules["det3d.core.sampler.preprocess"] = prep
    exec(compile(text, path, "exec"), prep.__dict__)
    sys.modules["det3d.core.sampler"].preprocess = prep
    ops = G._load_file("det3d.core.sampler.sample_ops", "det3d/core/sampler/sample_ops.py")
    pre.prep = prep
    return pre, prep, ops


class Recorder:
    """np.random's four entry points, wrapped while a sample runs"""

    def __init__(self):
        self.choice, self.uniform, self.normal, self.perm = [], [], [], None
        self._saved = {k: getattr(np.random, k) for k in ("choice", "uniform", "normal", "shuffle")}

    def __enter__(self):
        s = self._saved

        def choice(*a, **k):
            v = s["choice"](*a, **k)
            self.choice.append(bool(v))
            return v

        def uniform(*a, **k):
            v = s["uniform"](*a, **k)
            self.uniform.append(float(v))
            return v

        def normal(*a, **k):
            v = s["normal"](*a, **k)
            self.normal.append(float(np.asarray(v).reshape(-1)[0]))
            return v

        def shuffle(x):
            if np.ndim(x) == 2:                 # the points: the same swaps on an index list give the permutation
                state, before = np.random.get_state(), x.copy()
                idx = np.arange(len(x))
                s["shuffle"](idx)
                np.random.set_state(state)
                s["shuffle"](x)
                assert np.array_equal(x, before[idx], equal_nan=True)
                self.perm = idx
            else:
                s["shuffle"](x)
        np.random.choice, np.random.uniform, np.random.normal, np.random.shuffle = choice, uniform, normal, shuffle
        return self

    def __exit__(self, *exc):
        for k, v in self._saved.items():
            setattr(np.random, k, v)


def make_sampler(prep, ops, infos, groups, dtype):
    infos = copy.deepcopy(infos)
    for objs in infos.values():
        for o in objs:
            o["box3d_lidar"] = o["box3d_lidar"].astype(dtype)
    prepor = prep.DataBasePreprocessor([prep.DBFilterByMinNumPoint(A.DB_PREP[0]["filter_by_min_num_points"], logger=Log),
                                        prep.DBFilterByDifficulty(A.DB_PREP[1]["filter_by_difficulty"], logger=Log)])
    return ops.DataBaseSamplerV2(infos, groups, db_prepor=prepor, rate=1.0, global_rot_range=[0, 0], logger=Log)


def spy(sampler, index_of):
    """records what the samplers hand out and what sample_class_v2 keeps -> (offered [(index, group)], kept paths)"""
    offered, kept = [], []
    inner = sampler.sample_class_v2

    def sample_class_v2(name, num, gt_boxes):
        box = sampler._sampler_dict[name]
        take = box.sample

        def sample(n):
            got = take(n)
            offered.extend((index_of[o["path"]], sampler._sample_classes.index(name)) for o in got)
            return got
        box.sample = sample
        try:
            valid = inner(name, num, gt_boxes)
        finally:
            box.sample = take
        kept.extend(o["path"] for o in valid)
        return valid
    sampler.sample_class_v2 = sample_class_v2
    return offered, kept


def store(out, tag, name, f32, f64):
    if np.asarray(f32).size:
        GR.store(out, tag, name, f32, f64)
    else:
        out[f"{tag}_{name}_f32"], out[f"{tag}_{name}_diff"] = np.asarray(f32, np.float32), np.asarray(f32, np.float32)


def reference_matrix(prep, gt_boxes, cand_boxes):
    from det3d.core.bbox import box_np_ops
    total = np.concatenate([gt_boxes.reshape(-1, 9), cand_boxes.reshape(-1, 9)])
    bv = box_np_ops.center_to_corner_box2d(total[:, 0:2], total[:, 3:5], total[:, -1])
    m = prep.box_collision_test(bv, bv)
    m[np.arange(len(bv)), np.arange(len(bv))] = False
    return m[len(gt_boxes):]


def check_pairs(tag, gt_boxes, cand_boxes, excluded):
    """the restatement's decisions in float32 and float64, and their margins -> the float32 matrix"""
    t32, t64 = {}, {}
    m32 = A.collision_matrix(gt_boxes, cand_boxes, A.F32, traces=t32)
    m64 = A.collision_matrix(gt_boxes, cand_boxes, A.F64, traces=t64)
    for key in t64:
        bad = m32[key] != m64[key] or len(t32[key]) != len(t64[key])
        for (d32, _), (d64, s64) in zip(t32[key], t64[key]):
            bad |= not (abs(d64) > MARGIN * s64 or d32 == d64)
        if bad:
            excluded.append((tag, "pair") + key)
    return m32


def run_sample(pre, prep, ops, name, dtype, root):
    s = A.SAMPLES[name]
    scene, boxes, names = A.sample_inputs(name)
    infos, _ = A.database(s["F"])
    kept_db = A.kept_objects(infos)
    index_of = {o["path"]: i for i, (_, o) in enumerate(kept_db)}
    np.random.seed(s["seed"])
    sampler, offered, kept = None, [], []
    if s.get("sampler", True) and not s.get("no_augmentation", False):
        sampler = make_sampler(prep, ops, infos, A.GROUPS, dtype)
        offered, kept = spy(sampler, index_of)
    pre.build_dbsampler = lambda cfg: sampler
    cfg = Cfg(mode="train", shuffle_points=s.get("shuffle", True), global_rot_noise=s["rot"], global_scale_noise=A.SCALE_NOISE,
              global_translate_std=s["std"], class_names=A.CLASS_NAMES, db_sampler=sampler, no_augmentation=s.get("no_augmentation", False))
    stage = pre.Preprocess(cfg=cfg)
    res = dict(type="WaymoDataset", metadata=dict(image_prefix=root[s["F"]], num_point_features=s["F"]),
               lidar=dict(points=scene.astype(dtype), annotations=dict(boxes=boxes.astype(dtype), names=np.array(names, dtype=object).astype(str) if names else np.zeros(0, dtype="<U8"))))
    with Recorder() as rec:
        res, _ = stage(res, None)
    points_out = res["lidar"]["points"]
    ann = res["lidar"]["annotations"]
    before_filter = ann["gt_boxes"].copy()
    pc = np.asarray(A.PC_RANGE, np.float32)
    mask = prep.filter_gt_box_outside_range(ann["gt_boxes"], pc[[0, 1, 3, 4]])
    pre._dict_select(ann, mask)
    grid = np.round((pc[3:] - pc[:3]) / np.asarray(A.VOXEL, np.float32)).astype(np.int64)
    res["lidar"]["voxels"] = dict(shape=grid, range=pc, size=np.asarray(A.VOXEL, np.float32))
    acfg = Cfg(out_size_factor=8, target_assigner=Cfg(tasks=[Cfg(t) for t in A.TASKS]), gaussian_overlap=0.1, max_objs=A.MAX_OBJS, min_radius=2)
    res, _ = pre.AssignLabel(cfg=acfg)(res, None)
    gt_out = res["lidar"]["targets"]["gt_boxes_and_cls"]
    task_boxes = np.concatenate(res["lidar"]["annotations"]["gt_boxes"], 0)
    task_cls = pre.flatten(res["lidar"]["annotations"]["gt_classes"]) if len(task_boxes) else np.zeros(0)
    # (merge_multi_group_label has already added the tasks' offsets to these in place)
    full = np.zeros((A.MAX_OBJS, 10), np.float64)
    full[:len(task_boxes)] = np.concatenate([task_boxes, task_cls.reshape(-1, 1)], 1)[:, [0, 1, 2, 3, 4, 5, 8, 6, 7, 9]]
    assert np.array_equal(full.astype(np.float32), gt_out)
    draws = np.zeros(7)
    if not s.get("no_augmentation", False):
        assert len(rec.choice) == 2 and len(rec.uniform) == 2 and len(rec.normal) in (0, 3)
        draws[:2], draws[2:4] = rec.choice, rec.uniform
        draws[4:4 + len(rec.normal)] = rec.normal
    else:
        draws[3] = 1.0
    return dict(points=points_out, gt=full, count=len(task_boxes), offered=offered, kept=kept, kept_db=kept_db, draws=draws,
                perm=rec.perm, scene=scene, boxes=boxes, names=names, before_filter=before_filter, clouds=A.database(s["F"])[1])


def main():
    pre, prep, ops = import_reference()
    out, excluded = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        root = {}
        for F in (4, 5):
            root[F] = os.path.join(tmp, f"f{F}")
            A.write_database(root[F], *A.database(F))
        for name, s in A.SAMPLES.items():
            r32, r64 = (run_sample(pre, prep, ops, name, dt, root) for dt in (np.float32, np.float64))
            assert r32["offered"] == r64["offered"] and r32["kept"] == r64["kept"] and np.array_equal(r32["draws"], r64["draws"]), name
            assert (r32["perm"] is None) == (r64["perm"] is None) and (r32["perm"] is None or np.array_equal(r32["perm"], r64["perm"]))
            assert r32["points"].dtype == np.float32 and r64["points"].dtype == np.float64 and r32["count"] == r64["count"], name
            kept_db, names = r32["kept_db"], r32["names"]
            cand = np.array([i for i, _ in r32["offered"]], np.int64)
            group = np.array([g for _, g in r32["offered"]], np.int64)
            cand_boxes = np.stack([kept_db[i][1]["box3d_lidar"] for i in cand]) if len(cand) else np.zeros((0, 9), np.float32)
            cand_cls = [A.class_id(kept_db[i][0]) for i in cand]
            cand_rows = [r32["clouds"][kept_db[i][1]["path"]] for i in cand]
            ok = np.array([kept_db[i][1]["path"] in r32["kept"] for i in cand], bool)
            gt_cls = np.array([A.class_id(n) for n in names], np.int64)
            live = gt_cls >= 0
            # ---- the paste
            coll = reference_matrix(prep, r32["boxes"][live], cand_boxes)
            assert np.array_equal(coll, reference_matrix(prep, r32["boxes"][live].astype(np.float64), cand_boxes.astype(np.float64))), name
            mine = check_pairs(name, r32["boxes"][live], cand_boxes, excluded)
            assert np.array_equal(mine, coll), name
            assert np.array_equal(A.accept(coll, int(live.sum()), group), ok), name
            # ---- the draws as this project takes them
            xform = r32["draws"]
            rows = [len(c) for c in cand_rows]
            n_src, n_valid = sum(rows) + len(r32["scene"]), sum(r for r, a in zip(rows, ok) if a) + len(r32["scene"])
            keys = None
            if r32["perm"] is not None:
                assert len(r32["perm"]) == n_valid
                valid_src, at = [], 0
                for r, a in zip(rows, ok):
                    valid_src += list(range(at, at + r)) if a else []
                    at += r
                valid_src = np.array(valid_src + list(range(at, at + len(r32["scene"]))), np.int64)
                keys = np.full(n_src, -1, np.int64)
                keys[valid_src[r32["perm"]]] = np.arange(n_valid)
                keys[keys < 0] = n_valid + np.arange(n_src - n_valid)
                out[f"{name}_keys"] = keys.astype(np.int32)
            transform = not s.get("no_augmentation", False)
            # ---- the points
            m32, m64 = (A.points(r32["scene"], cand_rows, cand_boxes, ok, xform, keys, dt, transform)[:n_valid] if keys is not None else
                        A.points(r32["scene"], cand_rows, cand_boxes, ok, xform, None, dt, transform) for dt in (A.F32, A.F64))
            if keys is None:
                sel = ~np.isnan(m32[:, 0])
                m32, m64 = m32[sel], m64[sel]
            rotated = xform[2] != 0 and transform
            err = np.abs(m64 - r64["points"]).max() / max(np.abs(r64["points"]).max(), 1e-30) if m64.size else 0.0
            assert err < 1e-12, (name, err)
            if rotated:
                ratio, exact = A.column_ratio(m32, r32["points"], r64["points"])
                assert ratio <= A.BAR and exact, (name, ratio, exact)
            else:
                ratio = 0.0
                assert np.array_equal(m32, r32["points"]), name
            store(out, name, "points", r32["points"], r64["points"])
            # ---- the boxes
            margins = []
            b32, n32, _ = A.boxes(r32["boxes"], gt_cls, cand_boxes, cand_cls, ok, xform, dt=A.F32, transform=transform, margins=margins)
            b64, n64, _ = A.boxes(r32["boxes"], gt_cls, cand_boxes, cand_cls, ok, xform, dt=A.F64, transform=transform)
            for cross, scale in margins:
                if not abs(cross) > MARGIN * scale:
                    excluded.append((name, "range", cross, scale))
            assert n32 == n64 == r32["count"], (name, n32, n64, r32["count"])
            assert np.array_equal(b32[:, 9], r32["gt"][:, 9]) and np.array_equal(b64[:, 9], r64["gt"][:, 9]), name
            errb = np.abs(b64 - r64["gt"]).max() / max(np.abs(r64["gt"]).max(), 1e-30)
            assert errb < 1e-12, (name, errb)
            if rotated:
                rb, exact = A.column_ratio(b32[:n32], r32["gt"][:n32], r64["gt"][:n32])
                assert rb <= A.BAR and exact, (name, rb, exact)
            else:
                rb = 0.0
                assert np.array_equal(b32, r32["gt"].astype(np.float32)), name
            store(out, name, "gt", r32["gt"], r64["gt"])
            out[f"{name}_cand"], out[f"{name}_group"], out[f"{name}_coll"] = cand, group, coll.astype(np.uint8)
            out[f"{name}_accept"], out[f"{name}_xform"], out[f"{name}_count"] = ok.astype(np.uint8), xform, np.int64(r32["count"])
            print(f"{name}: {len(cand)} candidates, {int(ok.sum())} accepted, {int(coll.sum())} colliding pairs, {n_valid} of {n_src} rows valid, "
                  f"{r32['count']} boxes out; restatement fp32 ratio points {ratio:.2f} boxes {rb:.2f}, f64 err {err:.1e} / {errb:.1e}")
        # ---- the hand-made collision layouts, through sample_all with samplers that hand out everything in order
        for tag, gt, cands in A.collision_cases():
            gt = np.asarray(gt, np.float32).reshape(-1, 9)
            classes = [c for c in A.CLASS_NAMES if any(n == c for n, _ in cands)]
            infos = {c: [dict(name=c, path=f"col/{tag}_{c}_{i}.bin", box3d_lidar=np.asarray(b, np.float32), num_points_in_gt=9,
                              difficulty=0) for i, (n, b) in enumerate(cands) if n == c] for c in classes}
            os.makedirs(os.path.join(tmp, "col"), exist_ok=True)
            for objs in infos.values():
                for o in objs:
                    np.zeros((1, 5), np.float32).tofile(os.path.join(tmp, o["path"]))
            sampler = ops.DataBaseSamplerV2(infos, [{c: len(infos[c]) + len(gt) * (c == "VEHICLE")} for c in classes], rate=1.0,
                                            global_rot_range=[0, 0], logger=Log)
            for box in sampler._sampler_dict.values():
                box._indices, box._shuffle = np.arange(box._example_num), False
            order = [o["path"] for c in classes for o in infos[c]]
            offered, kept = spy(sampler, {p: i for i, p in enumerate(order)})
            sampler.sample_all(tmp, gt, np.array(["VEHICLE"] * len(gt)), 5)
            assert [i for i, _ in offered] == list(range(len(order))), tag
            cand_boxes = np.stack([o["box3d_lidar"] for c in classes for o in infos[c]])
            group = np.array([g for _, g in offered], np.int64)
            ok = np.array([p in kept for p in order], bool)
            coll = reference_matrix(prep, gt, cand_boxes)
            assert np.array_equal(check_pairs(tag, gt, cand_boxes, excluded), coll), tag
            assert np.array_equal(A.accept(coll, len(gt), group), ok), tag
            out[f"col_{tag}_coll"], out[f"col_{tag}_accept"] = coll.astype(np.uint8), ok.astype(np.uint8)
            print(f"collision case {tag}: matrix {coll.astype(int).tolist()}, accepted {ok.astype(int).tolist()}")
        # ---- the sampler alone, through a reset
        infos, _ = A.database(5)
        index_of = {o["path"]: i for i, (_, o) in enumerate(A.kept_objects(infos))}
        np.random.seed(99)
        sampler = make_sampler(prep, ops, infos, A.GROUPS, np.float32)
        seq, lens = [], []
        for call in range(6):
            names = ["VEHICLE"] * (call % 3) + ["PEDESTRIAN"] * (call % 2) + ["SIGN"]
            offered, _ = spy(sampler, index_of)
            sampler.sample_all(root[5], np.zeros((len(names), 9), np.float32) + 100 * np.arange(len(names), dtype=np.float32)[:, None], np.array(names), 5)
            sampler.sample_class_v2 = sampler.__class__.sample_class_v2.__get__(sampler)
            seq += [v for pair in offered for v in pair]
            lens.append(len(offered))
        out["seq_cand"], out["seq_len"] = np.array(seq, np.int64).reshape(-1, 2), np.array(lens, np.int64)
    print(f"excluded: {excluded}")
    assert len(excluded) <= MAX_EXCLUDED, excluded
    path = os.path.join(HERE, "augment.npz")
    G.save(path, out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
