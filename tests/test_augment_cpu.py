"""The training input without a GPU: tests/augment_ref.py's restatement against the reference's own record (tests/golden/
augment.npz, written by tests/golden/gen_augment.py), the planted faults, the sampler's bookkeeping against the reference's
recorded lists, the entries' declarations, their argument errors and the refusals of augment.py."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import augment_ref as A
from _common import ROOT, golden

hip = importlib.import_module("3dal_pytorch_amd._hip")
augment = importlib.import_module("3dal_pytorch_amd.augment")
detector = importlib.import_module("3dal_pytorch_amd.detector")

ENTRIES = ("dal3_gt_paste_select", "dal3_augment_points", "dal3_augment_points_workspace_bytes", "dal3_augment_boxes")
# the smallest factor by which a planted fault must move its measure (recorded below: the value faults move the worst column
# by 1e5 yardsticks and more; the discrete ones change at least one flag or row)
FAULT_RATIO = 1e3


@pytest.fixture(scope="module")
def gold():
    return golden("augment")


def recorded(g, name):
    """the archive's record of one sample beside its regenerated inputs"""
    s = A.SAMPLES[name]
    scene, boxes, names = A.sample_inputs(name)
    infos, clouds = A.database(s["F"])
    kept = A.kept_objects(infos)
    cand = g[f"{name}_cand"]
    r = dict(scene=scene, boxes=boxes, names=names, cand=cand, group=g[f"{name}_group"], coll=g[f"{name}_coll"].astype(bool),
             ok=g[f"{name}_accept"].astype(bool), xform=g[f"{name}_xform"], count=int(g[f"{name}_count"]),
             keys=g[f"{name}_keys"] if f"{name}_keys" in g else None, transform=not s.get("no_augmentation", False),
             cand_boxes=np.stack([kept[i][1]["box3d_lidar"] for i in cand]) if len(cand) else np.zeros((0, 9), np.float32),
             cand_cls=[A.class_id(kept[i][0]) for i in cand], cand_rows=[clouds[kept[i][1]["path"]] for i in cand],
             gt_cls=np.array([A.class_id(n) for n in names], np.int64))
    for k in ("points", "gt"):
        r[k] = g[f"{name}_{k}_f32"]
        r[k + "64"] = r[k].astype(np.float64) + g[f"{name}_{k}_diff"].astype(np.float64)
    r["n_valid"] = len(r["points"])
    return r


def restated_points(r, dt, fault=None):
    out = A.points(r["scene"], r["cand_rows"], r["cand_boxes"], r["ok"], r["xform"], r["keys"], dt, r["transform"], fault)
    return out[:r["n_valid"]] if r["keys"] is not None else out[~np.isnan(out[:, 0])]


def restated_boxes(r, dt, fault=None):
    return A.boxes(r["boxes"], r["gt_cls"], r["cand_boxes"], r["cand_cls"], r["ok"], r["xform"], dt=dt, transform=r["transform"], fault=fault)


@pytest.mark.parametrize("name", sorted(A.SAMPLES))
def test_restatement_equals_the_reference(gold, name):
    r = recorded(gold, name)
    live = r["gt_cls"] >= 0
    coll = A.collision_matrix(r["boxes"][live], r["cand_boxes"])
    assert np.array_equal(coll, r["coll"]) and np.array_equal(A.accept(coll, int(live.sum()), r["group"]), r["ok"])
    rotated = r["transform"] and r["xform"][2] != 0
    p32, p64 = restated_points(r, A.F32), restated_points(r, A.F64)
    b32, n32, over = restated_boxes(r, A.F32)
    b64, _, _ = restated_boxes(r, A.F64)
    assert n32 == r["count"] and not over and np.array_equal(b32[:, 9], r["gt"][:, 9]) and not b32[n32:].any()
    for mine64, want64 in ((p64, r["points64"]), (b64, r["gt64"])):
        assert mine64.shape == want64.shape
        assert not want64.size or np.abs(mine64 - want64).max() <= 1e-12 * max(np.abs(want64).max(), 1e-30)
    if rotated:                                 # within the archive's own float32-versus-float64 gap
        for mine, f32, truth in ((p32, r["points"], r["points64"]), (b32[:n32], r["gt"][:n32], r["gt64"][:n32])):
            ratio, exact = A.column_ratio(mine, f32, truth)
            assert ratio <= A.BAR and exact, (name, ratio, exact)
    else:                                       # flips, scale and translation: the same bits
        assert np.array_equal(p32, r["points"]) and np.array_equal(b32, r["gt"])


def test_golden_inputs_cover_the_cases(gold):
    r = {n: recorded(gold, n) for n in A.SAMPLES}
    assert {A.SAMPLES[n]["F"] for n in A.SAMPLES} == {4, 5} and {A.SAMPLES[n]["n"] for n in A.SAMPLES} >= {0, 1, 63, 64, 65, 3000}
    rows = [len(c) for v in r.values() for c in v["cand_rows"]]
    assert min(rows) >= 1 and max(rows) <= 200 and max(rows) > 150
    assert all(r[n]["coll"].any() and not r[n]["ok"].all() for n in ("s0", "s2", "s3", "s4", "s7")) and r["s1"]["ok"].all()
    assert len(r["s2"]["names"]) == 0 and len(r["s5"]["cand"]) == 0 and len(r["s6"]["cand"]) == 0
    assert 1 not in r["s3"]["group"].tolist()                # PEDESTRIAN's quota is met by the annotations
    flips = {(bool(v["xform"][0]), bool(v["xform"][1])) for v in r.values() if v["transform"]}
    assert len(flips) >= 3 and any(v["xform"][4:].any() for v in r.values())
    # a box with one corner inside the range stays, one wholly outside goes, a name outside class_names goes, an angle wraps
    s0 = r["s0"]
    c = A.corners(restated_unfiltered(s0))
    inside = [(abs(c[i, :, 0]) < 20).__and__(abs(c[i, :, 1]) < 16).sum() for i in range(2)]
    assert inside[0] == 1 and inside[1] == 0
    assert s0["count"] == int(s0["ok"].sum()) + 4 and 0 in s0["gt_cls"] and -1 in s0["gt_cls"]
    pre_wrap = restated_unfiltered(s0)[2, 8]
    assert abs(pre_wrap) > np.pi and np.abs(s0["gt"][:, 6]).max() <= np.pi
    # the hand-made layouts
    flags = {tag: gold[f"col_{tag}_accept"].tolist() for tag, _, _ in A.collision_cases()}
    assert flags["touching"] == [1, 1] and flags["inside"] == [0] and flags["contains"] == [0] and flags["chain_classes"] == [1, 0, 1]
    assert flags["forward"] == [0, 1] and flags["later_class"] == [1, 0, 1, 0] and flags["identical"] == [1, 1, 1]
    assert not gold["col_inside_coll"][0, 1:].any() and gold["col_inside_coll"][0, 0] == 1


def restated_unfiltered(r):
    """the boxes after the four transforms and before the range filter, GT rows first"""
    b, _, _ = A.boxes(r["boxes"], np.ones(len(r["boxes"]), np.int64), np.zeros((0, 9)), [], [], r["xform"], pc_range=[-1e6] * 3 + [1e6] * 3,
                      max_objs=len(r["boxes"]))
    out = b[:, [0, 1, 2, 3, 4, 5, 7, 8, 6]].copy()
    # undo limit_period for the angle: recompute it without the wrap
    x = r["xform"]
    rot = r["boxes"][:, 8].astype(np.float32)
    if x[0]:
        rot = -rot + np.float32(np.pi)
    if x[1]:
        rot = -rot + np.float32(2 * np.pi)
    out[:, 8] = rot + np.float32(x[2])
    return out


def test_the_margins_of_the_recorded_decisions(gold):
    """what gen_augment.py asserted when it wrote the archive, on the restatement alone: no decision within 1e-4 relative of
    its threshold unless float32 evaluates it exactly"""
    for name in A.SAMPLES:
        r = recorded(gold, name)
        live = r["gt_cls"] >= 0
        t32, t64 = {}, {}
        A.collision_matrix(r["boxes"][live], r["cand_boxes"], A.F32, traces=t32)
        A.collision_matrix(r["boxes"][live], r["cand_boxes"], A.F64, traces=t64)
        for key in t64:
            assert len(t32[key]) == len(t64[key])
            assert all(abs(d64) > 1e-4 * s64 or d32 == d64 for (d32, _), (d64, s64) in zip(t32[key], t64[key])), (name, key)
        margins = []
        A.boxes(r["boxes"], r["gt_cls"], r["cand_boxes"], r["cand_cls"], r["ok"], r["xform"], transform=r["transform"], margins=margins)
        assert all(abs(c) > 1e-4 * s for c, s in margins), name


def test_planted_faults_move_the_measures(gold):
    moved = {}
    # row and column not cleared on a reject: the forward layout accepts neither box
    for tag, gt, cands in A.collision_cases():
        coll = gold[f"col_{tag}_coll"].astype(bool)
        group = np.array([A.CLASS_NAMES.index(n) for n, _ in cands])
        group = np.unique(group, return_inverse=True)[1]
        good = A.accept(coll, len(gt), group)
        assert np.array_equal(good, gold[f"col_{tag}_accept"].astype(bool)), tag
        if tag in ("forward", "chain"):
            moved[f"no_clear/{tag}"] = int((A.accept(coll, len(gt), group, "no_clear") != good).sum())
        if tag in ("inside", "contains"):
            bad = A.collision_matrix(np.asarray(gt, np.float32), np.asarray([b for _, b in cands], np.float32), fault="no_containment")
            moved[f"no_containment/{tag}"] = int((bad != coll).sum())
    assert all(v >= 1 for v in moved.values()) and len(moved) == 4, moved
    # the value faults, in yardsticks of the worst column; the unstable rank in rows out of place
    ratios = {}
    for name in ("s0", "s3"):
        r = recorded(gold, name)
        n = r["count"]
        for fault in ("vel_not_flipped", "vel_not_scaled"):
            bad, _, _ = restated_boxes(r, A.F32, fault)
            ratios[f"{fault}/{name}"] = A.column_ratio(bad[:n], r["gt"][:n], r["gt64"][:n])[0]
    assert bool(recorded(gold, "s0")["xform"][:2].any()) and min(ratios.values()) >= FAULT_RATIO, ratios
    assert A.BAR < min(ratios.values()) / 10
    r = recorded(gold, "s1")
    keys = r["keys"] // 4                       # equal keys in runs of four
    r2 = dict(r, keys=keys, n_valid=len(keys))
    good, bad = restated_points(r2, A.F32), restated_points(r2, A.F32, "unstable_rank")
    assert int((good != bad).any(1).sum()) >= len(keys) // 2


def test_candidates_equal_the_reference_lists(gold, tmp_path):
    infos, clouds = A.database(5)
    path = A.write_database(str(tmp_path), infos, clouds)
    db = augment.GTDatabase(path, str(tmp_path), 5, A.DB_PREP, device="cpu")
    kept = A.kept_objects(infos)
    assert db.n == len(kept) and db.names == [n for n, _ in kept] and db.offsets[-1] == sum(len(clouds[o["path"]]) for _, o in kept)
    assert np.array_equal(db.boxes_host, np.stack([o["box3d_lidar"] for _, o in kept]))
    assert torch.equal(db.points, torch.from_numpy(np.concatenate([clouds[o["path"]] for _, o in kept])))
    # the sequence through a reset
    sampler = augment.DataBaseSamplerV2(db, A.GROUPS, rng=np.random.RandomState(99))
    got = []
    for call in range(6):
        names = ["VEHICLE"] * (call % 3) + ["PEDESTRIAN"] * (call % 2) + ["SIGN"]
        c = sampler.candidates(names)
        got.append([(i, g) for i, _, g in c])
        assert all(db.names[i] == n for i, n, _ in c)
    want, at = [], 0
    for n in gold["seq_len"]:
        want.append([tuple(v) for v in gold["seq_cand"][at:at + n].tolist()])
        at += n
    assert got == want and any(len(w) < 13 for w in want)
    # each sample's first call under its own seed
    for name, s in A.SAMPLES.items():
        if s["F"] != 5 or not s.get("sampler", True) or s.get("no_augmentation", False):
            continue
        sampler = augment.DataBaseSamplerV2(db, A.GROUPS, rng=np.random.RandomState(s["seed"]))
        c = sampler.candidates([n for n in s["names"] if n not in augment.DROPPED_NAMES])
        assert [i for i, _, _ in c] == gold[f"{name}_cand"].tolist() and [g for _, _, g in c] == gold[f"{name}_group"].tolist(), name


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dal3.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRIES:
        assert name + "(" in header and name in hip.SIGNATURES and hasattr(lib, name), name
    assert "DAL3_AUG_TOO_MANY = 32768, DAL3_AUG_OVERFLOW = 65536, DAL3_AUG_BAD_ROW = 131072" in header
    assert (hip.AUG_TOO_MANY, hip.AUG_OVERFLOW, hip.AUG_BAD_ROW) == (32768, 65536, 131072)
    assert f"#define DAL3_AUG_MAX_BOXES {hip.AUG_MAX_BOXES}" in header and f"#define DAL3_AUG_MAX_CAND {hip.AUG_MAX_CAND}" in header
    assert "dal3_augment.hip" in open(os.path.join(ROOT, "3dal_pytorch_amd", "csrc", "Makefile")).read()
    for struct, cls in (("dal3_gt_paste_args", hip.GtPasteArgs), ("dal3_augment_points_args", hip.AugmentPointsArgs),
                        ("dal3_augment_boxes_args", hip.AugmentBoxesArgs)):
        assert "} " + struct + ";" in header and cls.__doc__ == struct
    for name in ("GTDatabase", "BatchSampler", "DataBaseSamplerV2", "Draws", "make_draws", "Preprocess", "train_example"):
        assert hasattr(augment, name)
    assert callable(detector.VoxelNet.train_step_from_sweeps)


def test_argument_errors():
    lib = hip.lib()
    FAKE = 0x1000
    for fn in (lib.dal3_gt_paste_select, lib.dal3_augment_points, lib.dal3_augment_boxes):
        assert fn(None, None) == hip.EINVAL
    ok = dict(B=1, max_gt=4, max_cand=4)
    for bad, word in ((dict(B=-1), b"bad B"), (dict(B=65536), b"bad B"), (dict(max_gt=0), b"bad B"), (dict(max_gt=1025), b"bad B"),
                      (dict(max_cand=65), b"bad B"), (dict(), b"null argument")):
        assert lib.dal3_gt_paste_select(hip.GtPasteArgs(**dict(ok, **bad)), None) == hip.EINVAL and word in lib.dal3_last_error(), bad
    ok = dict(B=1, n=8, n_scene=8, F=5, max_cand=1, status=FAKE, workspace=FAKE, workspace_bytes=1 << 20)
    for bad, word in ((dict(B=-1), b"bad B"), (dict(n=1 << 31), b"bad B"), (dict(F=2), b"F 2"), (dict(F=9), b"F 9"), (dict(max_cand=0), b"max_cand"),
                      (dict(max_workgroups=-1), b"max_workgroups"), (dict(status=None), b"null status"), (dict(workspace=FAKE + 4), b"misaligned"),
                      (dict(), b"null argument")):
        assert lib.dal3_augment_points(hip.AugmentPointsArgs(**dict(ok, **bad)), None) == hip.EINVAL and word in lib.dal3_last_error(), bad
    full = dict(ok, out=FAKE, out_offsets=FAKE, scene_offsets=FAKE, cand_counts=FAKE, cand_seg_start=FAKE, cand_rows=FAKE, cand_db_row=FAKE,
                scene=FAKE)
    assert lib.dal3_augment_points(hip.AugmentPointsArgs(**dict(full, transform=1)), None) == hip.EINVAL and b"null argument" in lib.dal3_last_error()
    assert lib.dal3_augment_points(hip.AugmentPointsArgs(**dict(full, F=4, out=FAKE + 4)), None) == hip.EINVAL and b"16-byte" in lib.dal3_last_error()
    assert lib.dal3_augment_points(hip.AugmentPointsArgs(**dict(full, workspace_bytes=16)), None) == hip.EWORKSPACE
    need = lib.dal3_augment_points_workspace_bytes(4, 750000)
    assert need >= 2 * 8 * 750000 + 2 * 4 * 750000 and lib.dal3_augment_points_workspace_bytes(4, 1 << 31) == 0
    assert lib.dal3_augment_points_workspace_bytes(-1, 8) == 0
    ok = dict(B=1, max_gt=4, max_cand=4, max_objs=8, n_classes=3)
    for bad, word in ((dict(B=-1), b"bad B"), (dict(max_objs=0), b"max_objs"), (dict(max_objs=1025), b"max_objs"), (dict(n_classes=0), b"n_classes"),
                      (dict(n_classes=65), b"n_classes"), (dict(), b"null argument")):
        assert lib.dal3_augment_boxes(hip.AugmentBoxesArgs(**dict(ok, **bad)), None) == hip.EINVAL and word in lib.dal3_last_error(), bad


def test_refusals(tmp_path):
    cfg = dict(mode="train", shuffle_points=True, global_rot_noise=0.78, global_scale_noise=[0.95, 1.05], class_names=A.CLASS_NAMES, db_sampler=None)
    with pytest.raises(NotImplementedError, match="mode='train'"):
        augment.Preprocess(dict(cfg, mode="val"), pc_range=A.PC_RANGE)
    with pytest.raises(NotImplementedError, match="undefined name"):
        augment.Preprocess(dict(cfg, min_points_in_gt=5), pc_range=A.PC_RANGE)
    infos, clouds = A.database(5)
    path = A.write_database(str(tmp_path), infos, clouds)
    db = augment.GTDatabase(path, str(tmp_path), 5, A.DB_PREP, device="cpu")
    with pytest.raises(NotImplementedError, match="group sampling"):
        augment.DataBaseSamplerV2(db, [{"VEHICLE": 2, "CYCLIST": 2}])
    with pytest.raises(NotImplementedError, match="per-object noise"):
        augment.DataBaseSamplerV2(db, A.GROUPS, global_rot_range=[-0.3, 0.3])
    augment.DataBaseSamplerV2(db, A.GROUPS, global_rot_range=[0, 0])
    with pytest.raises(KeyError, match="SIGN"):
        augment.DataBaseSamplerV2(db, [{"SIGN": 2}])
    with pytest.raises(ValueError, match="not in class_names"):
        augment.Preprocess(dict(cfg, class_names=["VEHICLE"], db_sampler=augment.DataBaseSamplerV2(db, A.GROUPS)), pc_range=A.PC_RANGE)
    with pytest.raises(ValueError, match="unknown step"):
        augment.GTDatabase(path, str(tmp_path), 5, [dict(filter_by_colour=1)], device="cpu")
    with pytest.raises(ValueError):              # the objects' files hold five columns
        augment.GTDatabase(path, str(tmp_path), 4, device="cpu")
    assert augment.build_dbsampler(dict(enable=False), str(tmp_path), 5) is None and augment.build_dbsampler(None, None, 5) is None
    pre = augment.Preprocess(cfg, pc_range=A.PC_RANGE)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pre(torch.zeros(4, 5), [0, 4], torch.zeros(1, 1, 9), np.zeros((1, 1)), np.zeros(1))
    m = detector.VoxelNet.__new__(detector.VoxelNet)
    with pytest.raises(RuntimeError, match="set_train_input"):
        detector.VoxelNet.train_step_from_sweeps(m, None, None, {})
