"""The training input on the GPU (3dal_pytorch_amd/augment.py; dal3_gt_paste_select, dal3_augment_points, dal3_augment_boxes)
against the reference's own record, tests/golden/augment.npz: the collision decisions and the greedy acceptance exactly, the
points bit for bit without a rotation and per column against float64 with one (in multiples of the reference's own float32
error, augment_ref.BAR), gt_boxes_and_cls alike, the order of the rows, the chain into the voxeliser, the targets and the
loss. DAL3_AUGMENT_RECORD=<path> appends every measured ratio to that file (profiles/augment_measured.json)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import augment_ref as A
from _common import golden
from test_augment_cpu import recorded

hip = importlib.import_module("3dal_pytorch_amd._hip")
augment = importlib.import_module("3dal_pytorch_amd.augment")
pillars = importlib.import_module("3dal_pytorch_amd.pillars")
center_loss = importlib.import_module("3dal_pytorch_amd.center_loss")
pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    return golden("augment")


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    out = {}
    for F in (4, 5):
        root = str(tmp_path_factory.mktemp(f"db{F}"))
        out[F] = (A.write_database(root, *A.database(F)), root)
    return out


def _record(row, **values):
    path = os.environ.get("DAL3_AUGMENT_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(row=row, **values)) + "\n")


def _cfg(names, sampler):
    s = A.SAMPLES[names[0]]
    return dict(mode="train", shuffle_points=s.get("shuffle", True), global_rot_noise=0.78539816, global_scale_noise=A.SCALE_NOISE,
                global_translate_std=0.5, class_names=A.CLASS_NAMES, db_sampler=sampler, no_augmentation=s.get("no_augmentation", False))


def _batch(gold, names, roots, resident=True, keys_div=1, max_objs=A.MAX_OBJS):
    """the samples `names` as one batch -> (Preprocess, its arguments, the samples' records)"""
    rec = [recorded(gold, n) for n in names]
    F = A.SAMPLES[names[0]]["F"]
    db = augment.GTDatabase(roots[F][0], roots[F][1], F, A.DB_PREP, DEV, resident)
    sampler = augment.DataBaseSamplerV2(db, A.GROUPS, rng=np.random.RandomState(0))
    pre = augment.Preprocess(_cfg(names, sampler), pc_range=A.PC_RANGE, max_objs=max_objs)
    pre.keep_collisions = True
    max_gt = max(1, max(len(r["boxes"]) for r in rec))
    B = len(rec)
    gt_boxes, gt_cls, gt_cnt = np.zeros((B, max_gt, 9), np.float32), np.zeros((B, max_gt), np.int32), np.zeros(B, np.int32)
    for b, r in enumerate(rec):
        gt_boxes[b, :len(r["boxes"])], gt_cls[b, :len(r["boxes"])], gt_cnt[b] = r["boxes"], r["gt_cls"], len(r["boxes"])
    pts = np.concatenate([r["scene"] for r in rec])
    off = np.concatenate([[0], np.cumsum([len(r["scene"]) for r in rec])])
    cands = [[(int(i), db.names[int(i)], int(g)) for i, g in zip(r["cand"], r["group"])] for r in rec]
    keys = None
    if all(r["keys"] is not None for r in rec):
        keys = np.concatenate([r["keys"] // keys_div for r in rec])
    x = np.stack([r["xform"] for r in rec])
    draws = augment.Draws.from_values(x[:, 0], x[:, 1], x[:, 2], x[:, 3], x[:, 4:], keys, DEV)
    args = (torch.from_numpy(pts).to(DEV), off, torch.from_numpy(gt_boxes).to(DEV), gt_cls, gt_cnt, draws, cands)
    return pre, args, rec


@pytest.mark.parametrize("batch", sorted(A.BATCHES))
def test_batches_equal_the_reference(gold, roots, batch):
    names = A.BATCHES[batch]
    pre, args, rec = _batch(gold, names, roots)
    out, off, gt, status = pre(*args)
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and off[0] == 0 and out.shape[0] == off[-1]
    out, gt, counts = out.cpu().numpy(), gt.cpu().numpy(), pre.last["counts"].cpu().numpy()
    assert np.array_equal(pre.last["point_offsets_device"].cpu().numpy(), off)
    max_gt = args[2].shape[1]
    for b, r in enumerate(rec):
        n_src = sum(len(c) for c in r["cand_rows"]) + len(r["scene"])
        assert off[b + 1] - off[b] == n_src
        nc, live = len(r["cand"]), np.nonzero(r["gt_cls"] >= 0)[0]
        if nc:                                  # the pair matrix and the flags, exactly
            coll = pre.last["coll"][b].cpu().numpy().astype(bool)
            cols = np.concatenate([live, max_gt + np.arange(nc)])
            assert np.array_equal(coll[:nc][:, cols], r["coll"]), (batch, b)
            dead = np.setdiff1d(np.arange(coll.shape[1]), cols)
            assert not coll[:, dead].any() and not coll[nc:].any()
            assert np.array_equal(pre.last["accept"][b, :nc].cpu().numpy().astype(bool), r["ok"]), (batch, b)
        seg = out[off[b]:off[b + 1]]
        nan = np.isnan(seg).all(1)
        assert np.array_equal(nan, np.isnan(seg).any(1)) and int((~nan).sum()) == r["n_valid"]
        if r["keys"] is not None:               # the valid rows come first, in the archive's order; the rejected objects' rows are NaN
            assert not nan[:r["n_valid"]].any() and nan[r["n_valid"]:].all()
        got = seg[~nan]
        rotated = r["transform"] and r["xform"][2] != 0
        n = r["count"]
        assert counts[b] == n and np.array_equal(gt[b, :, 9], r["gt"][:, 9]) and not gt[b, n:].any()
        if rotated:
            ratio, exact = A.column_ratio(got, r["points"], r["points64"])
            rb, exact_b = A.column_ratio(gt[b, :n], r["gt"][:n], r["gt64"][:n])
            print(f"{batch}/{names[b]}: points {ratio:.3f} boxes {rb:.3f} yardsticks")
            _record(f"{batch}/{names[b]}", points=ratio, boxes=rb)
            assert exact and exact_b and ratio <= A.BAR and rb <= A.BAR, (batch, b, ratio, rb)
        else:
            assert np.array_equal(got, r["points"]), (batch, b)
            assert np.array_equal(gt[b], r["gt"]), (batch, b)


def test_collision_layouts_and_greedy_acceptance(gold, tmp_path):
    cases = A.collision_cases()
    infos, at, cands, cloud = {c: [] for c in A.CLASS_NAMES}, {}, [], {}
    for tag, _, cs in cases:
        for i, (name, box) in enumerate(cs):
            path = f"db/{tag}_{i}.bin"
            infos[name].append(dict(name=name, path=path, box3d_lidar=np.asarray(box, np.float32), num_points_in_gt=1, difficulty=0))
            cloud[path] = np.zeros((1, 5), np.float32)
    db = augment.GTDatabase(A.write_database(str(tmp_path), infos, cloud), str(tmp_path), 5, (), DEV)
    for name in A.CLASS_NAMES:
        for k, o in enumerate(infos[name]):
            at[o["path"]] = db.start[name] + k
    for tag, _, cs in cases:
        groups = np.unique([A.CLASS_NAMES.index(n) for n, _ in cs], return_inverse=True)[1]
        cands.append([(at[f"db/{tag}_{i}.bin"], n, int(groups[i])) for i, (n, _) in enumerate(cs)])
    B, max_gt = len(cases), 1
    gt_boxes, gt_cls, gt_cnt = np.zeros((B, max_gt, 9), np.float32), np.ones((B, max_gt), np.int32), np.zeros(B, np.int32)
    for b, (_, gt, _) in enumerate(cases):
        gt_boxes[b, :len(gt)], gt_cnt[b] = np.asarray(gt, np.float32).reshape(-1, 9), len(gt)
    cfg = dict(mode="train", shuffle_points=False, global_rot_noise=[0, 0], global_scale_noise=[1, 1], class_names=A.CLASS_NAMES,
               db_sampler=augment.DataBaseSamplerV2(db, [{c: 1} for c in A.CLASS_NAMES]))
    pre = augment.Preprocess(cfg, pc_range=[-100, -100, -3, 100, 100, 3], max_objs=8)
    pre.keep_collisions = True
    draws = augment.Draws.from_values(np.zeros(B), np.zeros(B), np.zeros(B), np.ones(B), np.zeros((B, 3)), None, DEV)
    out, off, gt, status = pre(torch.zeros((B, 5), device=DEV), np.arange(B + 1), torch.from_numpy(gt_boxes).to(DEV), gt_cls, gt_cnt, draws, cands)
    assert int(status.item()) == 0
    coll, ok, counts = pre.last["coll"].cpu().numpy(), pre.last["accept"].cpu().numpy(), pre.last["counts"].cpu().numpy()
    for b, (tag, g, cs) in enumerate(cases):
        nc, ng = len(cs), len(g)
        cols = np.concatenate([np.arange(ng), max_gt + np.arange(nc)]).astype(np.int64)
        assert np.array_equal(coll[b, :nc][:, cols], gold[f"col_{tag}_coll"]), tag
        assert np.array_equal(ok[b, :nc], gold[f"col_{tag}_accept"]), tag
        assert counts[b] == ng + int(gold[f"col_{tag}_accept"].sum()), tag
        rows = out[off[b]:off[b + 1]].cpu().numpy()
        assert np.array_equal(~np.isnan(rows[:nc, 0]), gold[f"col_{tag}_accept"].astype(bool)) and not np.isnan(rows[nc:]).any(), tag


def test_equal_keys_keep_source_order_across_sample_boundaries(gold, roots):
    # three copies of the unrotated sample, 1061 source rows each: both boundaries lie inside the first sort chunk of 4096
    pre, args, rec = _batch(gold, ["s1", "s1", "s1"], roots, keys_div=4)
    out, off, _, status = pre(*args)
    assert int(status.item()) == 0 and off[-1] < 4096
    out = out.cpu().numpy()
    for b, r in enumerate(rec):
        want = A.points(r["scene"], r["cand_rows"], r["cand_boxes"], r["ok"], r["xform"], r["keys"] // 4)
        assert np.array_equal(out[off[b]:off[b + 1]], want, equal_nan=True), b
    # and a boundary inside a later chunk, keys as recorded
    pre, args, rec = _batch(gold, ["s0", "s1"], roots, keys_div=4)
    out, off, _, _ = pre(*args)
    assert 4096 > off[1] > 3000 and off[2] > 4096
    r = rec[1]
    want = A.points(r["scene"], r["cand_rows"], r["cand_boxes"], r["ok"], r["xform"], r["keys"] // 4)
    assert np.array_equal(out[off[1]:off[2]].cpu().numpy(), want, equal_nan=True)


def test_resident_and_staged_database_and_reruns_give_the_same_bits(gold, roots):
    res = []
    for resident in (True, True, False):
        pre, args, _ = _batch(gold, A.BATCHES["A"], roots, resident=resident)
        out, off, gt, status = pre(*args)
        res.append((out, gt, pre.last["accept"], off))
    for other in res[1:]:
        assert torch.equal(res[0][0].view(torch.int32), other[0].view(torch.int32)) and torch.equal(res[0][1], other[1])
        assert torch.equal(res[0][2], other[2]) and np.array_equal(res[0][3], other[3])


def test_status_bits_and_host_limits(gold, roots):
    pre, args, rec = _batch(gold, ["s1"], roots, max_objs=5)
    _, _, gt, status = pre(*args)
    assert int(status.item()) == hip.AUG_OVERFLOW and int(pre.last["counts"][0]) == 5
    assert np.array_equal(gt[0].cpu().numpy(), rec[0]["gt"][:5])
    # more boxes than the pair matrix holds: the sample accepts nothing, keeps nothing and says so
    pre, args, rec = _batch(gold, ["s1"], roots)
    full = torch.zeros((1, hip.AUG_MAX_BOXES, 9), device=DEV)
    out, off, gt, status = pre(args[0], args[1], full, np.ones((1, hip.AUG_MAX_BOXES), np.int32), np.array([hip.AUG_MAX_BOXES], np.int32), args[5], args[6])
    assert int(status.item()) == hip.AUG_TOO_MANY and not pre.last["accept"].any() and int(pre.last["counts"][0]) == 0 and not gt.any()
    assert int((~torch.isnan(out[:, 0])).sum()) == len(rec[0]["scene"])
    pre, args, _ = _batch(gold, ["s1"], roots)
    many = [args[6][0] * 7]
    with pytest.raises(ValueError, match="at most 64"):
        pre(*args[:6], many)
    with pytest.raises(ValueError, match="order keys"):
        pre(*args[:5], augment.Draws(args[5].xform, args[5].keys[:-1]), args[6])
    with pytest.raises(TypeError, match="on the host"):
        pre(args[0], args[1], args[2], torch.from_numpy(args[3]).to(DEV), args[4])


def test_train_example_is_the_chain_of_its_stages(gold, roots):
    pre, args, _ = _batch(gold, A.BATCHES["A"], roots)
    acfg = dict(out_size_factor=8, target_assigner=dict(tasks=A.TASKS), gaussian_overlap=0.1, max_objs=A.MAX_OBJS, min_radius=2)
    assigner = center_loss.AssignLabel(cfg=acfg)
    kw = dict(voxel_size=A.VOXEL, pc_range=A.PC_RANGE, max_points=5, max_voxels=3000)
    ex = augment.train_example(pre, assigner, *args[:5], draws=args[5], candidates=args[6], **kw)
    pts, off, gt, _ = pre(*args)
    r = pillars.voxelize(pts, off, A.VOXEL, A.PC_RANGE, 5, 3000)
    grid = pillars.grid_size(A.VOXEL, A.PC_RANGE)
    tg = assigner(gt, voxels=dict(shape=grid, range=np.asarray(A.PC_RANGE, np.float32), size=np.asarray(A.VOXEL, np.float32)))
    assert int(ex["voxel_status"].item()) == 0 and int(ex["augment_status"].item()) == 0
    for k, want in (("voxels", r.voxels), ("coordinates", r.coordinates), ("num_points", r.num_points), ("n_voxels", r.n_pillars)):
        assert torch.equal(ex[k], want), k
    assert torch.equal(ex["num_voxels"], r.finish()[3]) and ex["shape"] == [[int(g) for g in grid]] * 2
    for k in ("hm", "anno_box", "ind", "mask", "cat"):
        assert all(torch.equal(a, b) for a, b in zip(ex[k], tg[k])), k
    # the voxels hold no NaN: the rejected objects' rows were dropped, and the live voxels are those of the valid rows alone
    m = int(r.voxel_offsets[-1])
    assert m > 0 and not torch.isnan(ex["voxels"][:m]).any()
    valid = pts[~torch.isnan(pts[:, 0])]
    n_valid = [int((~torch.isnan(pts[off[b]:off[b + 1], 0])).sum()) for b in range(2)]
    r2 = pillars.voxelize(valid.contiguous(), [0, n_valid[0], sum(n_valid)], A.VOXEL, A.PC_RANGE, 5, 3000)
    assert torch.equal(r2.voxel_offsets, r.voxel_offsets) and torch.equal(r2.voxels[:m], r.voxels[:m])


def test_train_step_from_sweeps_reaches_the_backbone(gold, roots):
    V = importlib.import_module("test_gpu_voxelnet")
    pts, off = V.sweep()
    db = augment.GTDatabase(roots[5][0], roots[5][1], 5, A.DB_PREP, DEV)
    cfg = dict(mode="train", shuffle_points=True, global_rot_noise=0.2, global_scale_noise=[0.95, 1.05], global_translate_std=0.1,
               class_names=A.CLASS_NAMES, db_sampler=augment.DataBaseSamplerV2(db, A.GROUPS, rng=np.random.RandomState(3)))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    pre = augment.Preprocess(cfg, pc_range=V.RANGE, max_objs=32, generator=gen)
    acfg = dict(out_size_factor=8, target_assigner=dict(tasks=V.TASKS), gaussian_overlap=0.1, max_objs=32, min_radius=2)
    m = V.detector.VoxelNet(**V.MODEL, **V.KW)
    m.load_state_dict(V.checkpoint(), strict=True)
    m = m.cuda().train()
    m.set_train_input(pre, center_loss.AssignLabel(cfg=acfg))
    gt = np.zeros((2, 2, 9), np.float32)
    gt[0, 0] = [-1.5, 1.0, 0.0, 1.8, 4.2, 1.6, 0.5, 0.1, 0.3]
    gt[0, 1] = [2.0, -2.5, 0.2, 0.7, 0.8, 1.7, 0, 0, -1.0]
    gt[1, 0] = [0.5, 2.5, -0.1, 0.6, 1.7, 1.5, 0, 0, 2.0]
    ann = dict(gt_boxes=torch.from_numpy(gt).to(DEV), gt_classes=np.array([[1, 2], [3, 0]], np.int32), gt_counts=np.array([2, 1], np.int32))
    out = m.train_step_from_sweeps(torch.from_numpy(pts).to(DEV) if isinstance(pts, np.ndarray) else pts.to(DEV), off, ann)
    loss = sum(out["loss"])
    loss.backward()
    assert bool(torch.isfinite(loss)) and int(m.last_example["augment_status"].item()) == 0
    g = next(p for n, p in m.backbone.named_parameters() if p.requires_grad and p.dim() > 1).grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert int(m.last_example["gt_counts"].sum()) >= 1


def test_make_draws_stay_within_the_config():
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    d = augment.make_draws(64, 5000, 0.785, [0.95, 1.05], [0.2, 0.3, 0.1], gen, DEV)
    x, k = d.xform.cpu().numpy(), d.keys.cpu().numpy()
    assert k.dtype == np.int32 and k.shape == (5000,) and k.min() >= 0 and len(np.unique(k)) > 4900
    assert set(np.unique(x[:, :2])) == {0.0, 1.0} and np.abs(x[:, 2]).max() <= 0.785 and x[:, 3].min() >= 0.95 and x[:, 3].max() <= 1.05
    assert x[:, 2].std() > 0.2 and 0.1 < x[:, 4].std() < 0.3 and np.abs(x[:, 4:]).max() < 2
    d = augment.make_draws(4, 10, [0, 0], [1, 1], 0, gen, DEV, shuffle=False)
    assert d.keys is None and not d.xform[:, 2].any() and bool((d.xform[:, 3] == 1).all()) and not d.xform[:, 4:].any()
