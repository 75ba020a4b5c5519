"""The detector's training input on the GPU through lib3dal_hip.so (dal3_gt_paste_select, dal3_augment_points,
dal3_augment_boxes, include/dal3.h), under the reference's names: `Preprocess` in train mode (det3d/datasets/pipelines/
preprocess.py) with the ground-truth paste of `DataBaseSamplerV2.sample_all` (det3d/core/sampler/sample_ops.py),
`random_flip_both`, `global_rotation`, `global_scaling_v2`, `global_translate_` and the point shuffle (det3d/core/sampler/
preprocess.py), `Voxelization`'s `filter_gt_box_outside_range` and `AssignLabel`'s regrouping into `gt_boxes_and_cls`.

The reference does this per sample in numba on DataLoader workers. Here a batch of resident sweeps and annotations becomes
the `example` that `VoxelNet.first_stage_loss` takes, enqueued on the current stream with no host synchronisation:

  host     the integer bookkeeping of the sampler (`BatchSampler`, `DataBaseSamplerV2.candidates`): which database objects
           are offered to which sample. It depends on the class counts of the annotations alone, so it is known before any
           device decision, and with it every size: sample b's output segment holds its scene rows and ALL of its
           candidates' rows, accepted or not.
  device   which candidates collide (dal3_gt_paste_select), the points (dal3_augment_points: a rejected candidate's rows are
           written as NaN rows, which dal3_voxelize drops, so `point_offsets` stays a host array of capacities, as
           `pillars.voxelize` requires) and the boxes (dal3_augment_boxes).

Nothing is read back. What goes up per step is small and comes from pageable host memory, as `pillars.voxelize`'s offsets do:
the step's bookkeeping in one int64 array, and the annotations' classes and counts when they are given as host arrays.

The step's randomness is an input (`Draws`), as two_stage's is: `make_draws` fills it on the device from a torch.Generator,
the golden tests pass the values the reference drew.

Not built: Preprocess in val mode, `min_points_in_gt > 0` (the reference's branch reads an undefined name), group sampling,
`random_crop`, per-object noise (refused unless its range is degenerate, as the Waymo configs set it), and a
`train_step_from_sweeps` for PointPillars.
"""
import os
import pickle

import numpy as np
import torch

from . import _hip, pillars

DROPPED_NAMES = ("DontCare", "ignore", "UNKNOWN")       # Preprocess removes these before it samples


def _get(cfg, key, *default):
    if isinstance(cfg, dict):
        return cfg[key] if not default or key in cfg else default[0]
    return getattr(cfg, key, *default)


def _items(step):
    return step.items() if isinstance(step, dict) else dict(step).items()


class GTDatabase:
    """The object database of `create_groundtruth_database`: `dbinfos_*.pkl` (class name -> list of {name, path, box3d_lidar,
    num_points_in_gt, difficulty, ..}) filtered by `db_prep_steps` (the config's list of {filter_by_min_num_points: {name:
    n}} / {filter_by_difficulty: [..]}, applied in its order) and every kept object's `.bin` loaded ONCE into one packed
    float32 tensor (total, F) with int64 `offsets` (n + 1). `boxes` (n, 9) float32 lives on the device; `names[i]` is object
    i's class, `start[name]` .. `start[name] + count[name]` the objects of a class. resident=True keeps the packed points on
    the device; resident=False keeps them in pinned host memory and `stage` copies a step's candidates' rows with
    non_blocking=True."""

    def __init__(self, db_info_path, root_path, num_point_features, db_prep_steps=(), device="cuda", resident=True):
        with open(db_info_path, "rb") as f:
            infos = pickle.load(f)
        infos = {k: list(v) for k, v in infos.items()}
        for step in db_prep_steps or ():
            for kind, arg in _items(step):
                if kind == "filter_by_min_num_points":
                    for name, min_num in _items(arg):
                        if min_num > 0:
                            infos[name] = [i for i in infos[name] if i["num_points_in_gt"] >= min_num]
                elif kind == "filter_by_difficulty":
                    infos = {k: [i for i in v if i["difficulty"] not in arg] for k, v in infos.items()}
                else:
                    raise ValueError(f"db_prep_steps: unknown step {kind!r}")
        self.F = int(num_point_features)
        if not 3 <= self.F <= 8:
            raise ValueError(f"num_point_features = {self.F}: 3 .. 8")
        self.device, self.resident = torch.device(device), bool(resident)
        self.names, self.start, self.count = [], {}, {}
        boxes, clouds, offsets = [], [], [0]
        for name, objs in infos.items():
            self.start[name], self.count[name] = len(self.names), len(objs)
            for info in objs:
                if "rot_transform" in info:
                    raise ValueError("a database entry carries rot_transform: per-object rotation is not built")
                box = np.asarray(info["box3d_lidar"], dtype=np.float32).reshape(-1)
                if box.size != 9:
                    raise ValueError(f"box3d_lidar of {info['path']} has {box.size} columns, 9 expected (x, y, z, w, l, h, vx, vy, rot)")
                pts = np.fromfile(os.path.join(str(root_path), info["path"]), dtype=np.float32).reshape(-1, self.F)
                self.names.append(info["name"])
                boxes.append(box)
                clouds.append(pts)
                offsets.append(offsets[-1] + pts.shape[0])
        self.n = len(self.names)
        self.offsets = np.asarray(offsets, dtype=np.int64)
        packed = torch.from_numpy(np.concatenate(clouds, 0) if clouds else np.zeros((0, self.F), np.float32))
        self.boxes_host = np.stack(boxes) if boxes else np.zeros((0, 9), np.float32)
        self.boxes = torch.from_numpy(self.boxes_host).to(self.device)
        if self.resident:
            self.points = packed.to(self.device)
        else:
            self.points = packed.pin_memory() if self.device.type == "cuda" else packed

    def stage(self, index):
        """the packed rows of the objects `index` (a host int64 array) for one step -> (points (rows, F) on the device, first
        row of each object in it). Resident: the database itself and its own offsets, nothing is copied."""
        index = np.asarray(index, dtype=np.int64)
        if self.resident:
            return self.points, self.offsets[index]
        rows = self.offsets[index + 1] - self.offsets[index]
        first = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        out = torch.empty((max(int(first[-1]), 1), self.F), dtype=torch.float32, device=self.device)
        for k, i in enumerate(index):
            if rows[k]:
                out[first[k]:first[k + 1]].copy_(self.points[self.offsets[i]:self.offsets[i + 1]], non_blocking=True)
        return out, first[:-1]


class BatchSampler:
    """det3d/core/sampler/preprocess.py's BatchSampler over n indices: a shuffled index list that hands out the next `num`
    and, when fewer than num + 1 are left, the rest, after which it is shuffled again. Draws from `rng` (a
    numpy.random.RandomState) where the reference draws from numpy's global state."""

    def __init__(self, n, rng, shuffle=True):
        self._indices = np.arange(int(n))
        self._rng, self._shuffle, self._idx, self._n = rng, shuffle, 0, int(n)
        if shuffle:
            rng.shuffle(self._indices)

    def sample(self, num):
        if self._idx + num >= self._n:
            ret = self._indices[self._idx:].copy()
            if self._shuffle:
                self._rng.shuffle(self._indices)
            self._idx = 0
        else:
            ret = self._indices[self._idx:self._idx + num]
            self._idx += num
        return ret


class DataBaseSamplerV2:
    """The integer bookkeeping of sample_ops.py's DataBaseSamplerV2 over a `GTDatabase`. groups: the config's sample_groups, a
    list of {class name: max number}; rate as the reference's. `candidates(gt_names)` is sample_all up to the collision test:
    per group in order, sampled_num = round(rate * (max - count of the name among gt_names)) and, when positive, the
    sampler's next indices of that class. The collision test and everything after it runs on the device."""

    def __init__(self, db, groups, rate=1.0, global_rot_range=None, rng=None):
        if any(len(g) > 1 for g in groups):
            raise NotImplementedError("group sampling (a sample group of several classes) is not built")
        if global_rot_range is not None:
            r = global_rot_range if isinstance(global_rot_range, (list, tuple, np.ndarray)) else [-global_rot_range, global_rot_range]
            if abs(r[0] - r[1]) >= 1e-3:
                raise NotImplementedError("global_random_rotation_range_per_object: per-object noise is not built; the range must "
                                          "be degenerate ([0, 0], as the Waymo configs set it)")
        self.db, self.rate = db, rate
        self.sample_classes = [k for g in groups for k in g.keys()]
        self.sample_max_nums = [v for g in groups for v in g.values()]
        rng = np.random.RandomState() if rng is None else rng
        for name in self.sample_classes:
            if name not in db.start:
                raise KeyError(f"sample group {name!r} is not a class of the database")
        # one sampler per class of the database, made in the database's order: the order the reference shuffles them in
        self._samplers = {name: BatchSampler(db.count[name], rng) for name in db.start}

    def candidates(self, gt_names):
        """-> [(database index, class name, group)] in group order"""
        out = []
        for g, (name, max_num) in enumerate(zip(self.sample_classes, self.sample_max_nums)):
            num = int(max_num - np.sum([n == name for n in gt_names]))
            num = int(np.round(self.rate * num).astype(np.int64))
            if num > 0:
                out += [(self.db.start[name] + int(i), name, g) for i in self._samplers[name].sample(num)]
        return out


def build_dbsampler(cfg, root_path, num_point_features, device="cuda", rng=None, resident=True):
    """det3d/builder.py's build_dbsampler from the config's dict (db_info_path, sample_groups, db_prep_steps, rate,
    global_random_rotation_range_per_object, enable) -> DataBaseSamplerV2, or None when `enable` is false"""
    if cfg is None or not _get(cfg, "enable", True):
        return None
    db = GTDatabase(_get(cfg, "db_info_path"), root_path, num_point_features, _get(cfg, "db_prep_steps", ()), device, resident)
    return DataBaseSamplerV2(db, _get(cfg, "sample_groups"), _get(cfg, "rate", 1.0),
                             _get(cfg, "global_random_rotation_range_per_object", None), rng)


class Draws:
    """One step's randomness on the device. xform (B, 7) float64: the y-flip and x-flip flags (0 / 1, random_flip_both's two
    draws in its order), noise_rotation, noise_scale, noise_translate (3; zero when the std is 0). keys (n) int32: one
    31-bit order key per source row, or None for the identity order."""

    def __init__(self, xform, keys):
        self.xform, self.keys = xform, keys

    @classmethod
    def from_values(cls, flip_y, flip_x, rotation, scale, translate, keys, device):
        B = len(rotation)
        x = np.zeros((B, 7), np.float64)
        x[:, 0], x[:, 1], x[:, 2], x[:, 3] = flip_y, flip_x, rotation, scale
        x[:, 4:] = np.asarray(translate, np.float64).reshape(B, 3)
        keys = None if keys is None else torch.as_tensor(np.asarray(keys, np.int32)).to(device)
        return cls(torch.from_numpy(x).to(device), keys)


def make_draws(B, n_rows, rot_noise, scale_noise, translate_std, generator, device, shuffle=True):
    """the reference's draws from a torch.Generator on `device`: flips with probability 0.5, noise_rotation uniform over
    [-r, r] (or the list's bounds), noise_scale uniform over scale_noise, noise_translate normal with std (x, y, x) as
    global_translate_ has it, and a random 31-bit order key per source row. Nothing is read back."""
    rot = list(rot_noise) if isinstance(rot_noise, (list, tuple)) else [-rot_noise, rot_noise]
    std = translate_std if isinstance(translate_std, (list, tuple, np.ndarray)) else [translate_std] * 3
    u = torch.rand((B, 4), generator=generator, device=device, dtype=torch.float64)
    x = torch.zeros((B, 7), dtype=torch.float64, device=device)
    x[:, 0:2] = (u[:, 0:2] < 0.5).double()
    x[:, 2] = rot[0] + (rot[1] - rot[0]) * u[:, 2]
    x[:, 3] = scale_noise[0] + (scale_noise[1] - scale_noise[0]) * u[:, 3]
    if any(e != 0 for e in std):
        z = torch.randn((B, 3), generator=generator, device=device, dtype=torch.float64)
        x[:, 4:] = z * torch.tensor([std[0], std[1], std[0]], dtype=torch.float64, device=device)
    keys = None
    if shuffle:
        keys = torch.randint(0, 2 ** 31, (max(int(n_rows), 1),), generator=generator, device=device).to(torch.int32)[:int(n_rows)]
    return Draws(x, keys)


class Preprocess:
    """pipelines/preprocess.py's Preprocess with its config keys (mode="train", shuffle_points, global_rot_noise,
    global_scale_noise, global_translate_std, db_sampler, class_names, no_augmentation). pc_range: the voxeliser's range;
    Voxelization's filter_gt_box_outside_range and AssignLabel's regrouping are folded into the boxes' kernel. db_sampler:
    None, a DataBaseSamplerV2, or the config's dict (then root_path and num_point_features say where the database lies).
    max_objs: AssignLabel's.

    __call__(points (N, F) float32 CUDA, point_offsets (B + 1) host, gt_boxes (B, max_gt, 9) float32 CUDA [x, y, z, w, l, h,
    vx, vy, rot], gt_classes (B, max_gt), gt_counts (B), draws=None) -> (points' (n, F), point_offsets' (B + 1) host int64,
    gt_boxes_and_cls (B, max_objs, 10), status (1) int32). gt_classes: the 1-based index into class_names, 0 for another
    name, negative for a name of DROPPED_NAMES; with a sampler it and gt_counts are HOST arrays (the annotations come from
    the host, and the candidates are drawn from the class counts), else they may be device tensors. `last` keeps
    point_offsets_device, counts (B), accept, the candidates and, with keep_collisions, the pair matrix."""

    def __init__(self, cfg=None, *, pc_range, max_objs=500, root_path=None, num_point_features=None, device="cuda", rng=None,
                 generator=None, **kwargs):
        self.mode = _get(cfg, "mode")
        if self.mode != "train":
            raise NotImplementedError("Preprocess: only mode='train' is built (val mode passes the points through)")
        if _get(cfg, "min_points_in_gt", -1) > 0:
            raise NotImplementedError("min_points_in_gt > 0: the reference's branch reads an undefined name (min_points_in_gt "
                                      "without self.) and cannot run; it is not built")
        self.shuffle_points = bool(_get(cfg, "shuffle_points"))
        self.no_augmentation = bool(_get(cfg, "no_augmentation", False))
        self.global_rotation_noise = _get(cfg, "global_rot_noise")
        self.global_scaling_noise = _get(cfg, "global_scale_noise")
        self.global_translate_std = _get(cfg, "global_translate_std", 0)
        self.class_names = list(_get(cfg, "class_names"))
        if not 1 <= len(self.class_names) <= _hip.CENTER_MAX_CLASSES:
            raise ValueError(f"class_names: 1 .. {_hip.CENTER_MAX_CLASSES} classes")
        sampler = _get(cfg, "db_sampler", None)
        if sampler is not None and not isinstance(sampler, DataBaseSamplerV2):
            sampler = build_dbsampler(sampler, root_path, num_point_features, device, rng)
        if sampler is not None:
            for name in sampler.db.names:
                if name not in self.class_names:
                    raise ValueError(f"the database holds class {name!r}, which is not in class_names (the reference fails on it)")
        self.db_sampler = sampler
        r = np.asarray(pc_range, dtype=np.float32).reshape(-1)
        self.bv_range = [float(v) for v in (r[[0, 1, 3, 4]] if r.size == 6 else r)]
        self.max_objs = int(max_objs)
        self.generator, self.keep_collisions, self.last = generator, False, None

    def candidates(self, gt_classes, gt_counts):
        """the sampler's candidates for a batch from the HOST class ids -> per sample [(database index, name, group)]"""
        out = []
        for b in range(len(gt_counts)):
            ids = np.asarray(gt_classes[b][:int(gt_counts[b])])
            names = [self.class_names[i - 1] if i >= 1 else None for i in ids[ids >= 0]]
            out.append(self.db_sampler.candidates(names))
        return out

    def __call__(self, points, point_offsets, gt_boxes, gt_classes, gt_counts, draws=None, candidates=None):
        for t, what in ((points, "points"), (gt_boxes, "gt_boxes")):
            if not torch.is_tensor(t):
                raise TypeError(f"{what} must be a tensor")
            _hip.require_gpu(t, what)
        if points.dim() != 2 or points.dtype != torch.float32 or not 3 <= points.shape[1] <= 8:
            raise ValueError(f"points must be float32 (N, 3 .. 8), got {points.dtype} {tuple(points.shape)}")
        if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 9 or gt_boxes.dtype != torch.float32 or not 1 <= gt_boxes.shape[1] <= _hip.AUG_MAX_BOXES:
            raise ValueError(f"gt_boxes must be float32 (B, 1 .. {_hip.AUG_MAX_BOXES}, 9), got {gt_boxes.dtype} {tuple(gt_boxes.shape)}")
        points, gt_boxes = points.contiguous(), gt_boxes.contiguous()
        N, F = points.shape
        dev = points.device
        off = _hip.host_offsets(point_offsets, N, "point_offsets", "the capacity of the outputs comes", "B")
        B, max_gt = off.size - 1, gt_boxes.shape[1]
        if gt_boxes.shape[0] != B:
            raise ValueError(f"gt_boxes holds {gt_boxes.shape[0]} samples, point_offsets {B}")
        sampler = None if self.no_augmentation else self.db_sampler
        if sampler is not None and candidates is None:
            if torch.is_tensor(gt_classes) and gt_classes.is_cuda or torch.is_tensor(gt_counts) and gt_counts.is_cuda:
                raise TypeError("with a db_sampler gt_classes and gt_counts must be on the host: the candidates are drawn from the "
                                "class counts, and reading a device tensor back would be the synchronisation this call avoids")
            candidates = self.candidates(np.asarray(gt_classes), np.asarray(gt_counts))
        if sampler is None:
            candidates = [[] for _ in range(B)]
        if len(candidates) != B:
            raise ValueError(f"candidates for {len(candidates)} samples, the batch has {B}")
        if sampler is not None and sampler.db.F != F:
            raise ValueError(f"the database's objects have {sampler.db.F} point features, the sweeps {F}")
        cls_d, cnt_d = (torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).to(dev).to(torch.int32).contiguous()
                        for t in (gt_classes, gt_counts))
        if tuple(cls_d.shape) != (B, max_gt) or tuple(cnt_d.shape) != (B,):
            raise ValueError(f"gt_classes must be ({B}, {max_gt}) and gt_counts ({B},), got {tuple(cls_d.shape)}, {tuple(cnt_d.shape)}")
        MC = max(1, max(len(c) for c in candidates)) if B else 1
        if MC > _hip.AUG_MAX_CAND:
            raise ValueError(f"{MC} candidates for one sample: at most {_hip.AUG_MAX_CAND} (DAL3_AUG_MAX_CAND)")
        # the step's host bookkeeping, one upload: offsets, and per candidate its rows, group, class and database index
        flat = np.asarray([i for c in candidates for i, _, _ in c], dtype=np.int64)
        if flat.size:
            db = sampler.db
            db_points, first = db.stage(flat)
            rows_flat = db.offsets[flat + 1] - db.offsets[flat]
        else:
            db_points, first, rows_flat = None, np.zeros(0, np.int64), np.zeros(0, np.int64)
        at, where = 0, {}
        for name, size in (("out_off", B + 1), ("scene_off", B + 1), ("cand_cnt", B), ("seg", B * MC), ("rows", B * MC),
                           ("dbrow", B * MC), ("group", B * MC), ("klass", B * MC), ("index", B * MC)):
            where[name] = slice(at, at + size)
            at += size
        meta = np.zeros(at, np.int64)
        out_off, scene_off, cand_cnt = (meta[where[k]] for k in ("out_off", "scene_off", "cand_cnt"))
        seg, rows, dbrow, group, klass, index = (meta[where[k]].reshape(B, MC) for k in ("seg", "rows", "dbrow", "group", "klass", "index"))
        scene_off[:] = off
        k = 0
        for b in range(B):
            cand_cnt[b] = len(candidates[b])
            at = out_off[b]
            for i, (idx, name, g) in enumerate(candidates[b]):
                seg[b, i], rows[b, i], dbrow[b, i], group[b, i], index[b, i] = at, rows_flat[k], first[k], g, idx
                klass[b, i] = self.class_names.index(name) + 1
                at += rows_flat[k]
                k += 1
            out_off[b + 1] = at + (off[b + 1] - off[b])
        n = int(out_off[B])
        if n >= 2 ** 31:
            raise ValueError("2^31 or more source rows: split the batch")
        out_off_host = out_off.copy()
        meta_d = torch.from_numpy(meta).to(dev)
        part = lambda name: meta_d[where[name]]                 # noqa: E731
        transform = 0 if self.no_augmentation else 1
        if draws is None:
            draws = make_draws(B, n, self.global_rotation_noise, self.global_scaling_noise, self.global_translate_std,
                               self.generator, dev, self.shuffle_points) if transform or self.shuffle_points else Draws(None, None)
        keys = draws.keys if self.shuffle_points else None
        if keys is not None and (keys.dtype != torch.int32 or keys.numel() != n or not keys.is_cuda):
            raise ValueError(f"draws.keys must be a CUDA int32 tensor of {n} order keys (one per source row)")
        xform = draws.xform if transform else None
        if transform and (xform is None or xform.dtype != torch.float64 or tuple(xform.shape) != (B, 7) or not xform.is_cuda):
            raise ValueError(f"draws.xform must be a CUDA float64 ({B}, 7) tensor")
        lib = _hip.lib()
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        accept = coll = cand_boxes = None
        if flat.size:
            cand_boxes = sampler.db.boxes.index_select(0, part("index"))
            accept = torch.empty((B, MC), dtype=torch.uint8, device=dev)
            if self.keep_collisions:
                coll = torch.zeros((B, MC, max_gt + MC), dtype=torch.uint8, device=dev)
            a = _hip.GtPasteArgs(B=B, max_gt=max_gt, max_cand=MC, gt_boxes=_hip.ptr(gt_boxes), gt_classes=_hip.ptr(cls_d),
                                 gt_counts=_hip.ptr(cnt_d), cand_boxes=_hip.ptr(cand_boxes), cand_group=_hip.ptr(part("group")),
                                 cand_counts=_hip.ptr(part("cand_cnt")), accept=_hip.ptr(accept), coll=_hip.ptr(coll),
                                 status=_hip.ptr(status))
            _hip.check(lib.dal3_gt_paste_select(a, _hip.stream()))
        out = torch.empty((n, F), dtype=torch.float32, device=dev)
        nbytes = lib.dal3_augment_points_workspace_bytes(B, n)
        ws = _hip.workspace(nbytes, dev)
        a = _hip.AugmentPointsArgs(B=B, n=n, n_scene=N, db_rows=0 if db_points is None else db_points.shape[0], F=F,
                                   transform=transform, max_cand=MC, scene=_hip.ptr(points), scene_offsets=_hip.ptr(part("scene_off")),
                                   db_points=_hip.ptr(db_points), out_offsets=_hip.ptr(part("out_off")),
                                   cand_counts=_hip.ptr(part("cand_cnt")), cand_seg_start=_hip.ptr(part("seg")),
                                   cand_rows=_hip.ptr(part("rows")), cand_db_row=_hip.ptr(part("dbrow")), cand_boxes=_hip.ptr(cand_boxes),
                                   accept=_hip.ptr(accept), keys=_hip.ptr(keys), xform=_hip.ptr(xform), out=_hip.ptr(out),
                                   status=_hip.ptr(status), max_workgroups=0, workspace=_hip.ptr(ws), workspace_bytes=ws.numel())
        _hip.check(lib.dal3_augment_points(a, _hip.stream()))
        gt = torch.empty((B, self.max_objs, 10), dtype=torch.float32, device=dev)
        counts = torch.empty(B, dtype=torch.int32, device=dev)
        a = _hip.AugmentBoxesArgs(B=B, max_gt=max_gt, max_cand=MC, max_objs=self.max_objs, n_classes=len(self.class_names),
                                  transform=transform, gt_boxes=_hip.ptr(gt_boxes), gt_classes=_hip.ptr(cls_d),
                                  gt_counts=_hip.ptr(cnt_d), cand_boxes=_hip.ptr(cand_boxes), cand_classes=_hip.ptr(part("klass")),
                                  cand_counts=_hip.ptr(part("cand_cnt")), accept=_hip.ptr(accept), xform=_hip.ptr(xform),
                                  out=_hip.ptr(gt), out_count=_hip.ptr(counts), status=_hip.ptr(status))
        a.range[:] = self.bv_range
        _hip.check(lib.dal3_augment_boxes(a, _hip.stream()))
        self.last = dict(point_offsets_device=part("out_off"), counts=counts, accept=accept, candidates=candidates, coll=coll,
                         draws=draws)
        return out, out_off_host, gt, status


def train_example(preprocess, assigner, points, point_offsets, gt_boxes, gt_classes, gt_counts, *, voxel_size, pc_range,
                  max_points, max_voxels, draws=None, candidates=None):
    """Preprocess -> pillars.voxelize -> center_loss.AssignLabel: the dictionary VoxelNet.first_stage_loss takes, every
    entry a device tensor of capacity size (`n_voxels` is the device count of the live voxels), on the current stream with
    no host synchronisation. Also: gt_boxes_and_cls, gt_counts, augment_status, voxel_status."""
    pts, off, gt, status = preprocess(points, point_offsets, gt_boxes, gt_classes, gt_counts, draws, candidates)
    r = pillars.voxelize(pts, off, voxel_size, pc_range, max_points, max_voxels,
                         point_offsets_device=preprocess.last["point_offsets_device"])
    grid = pillars.grid_size(voxel_size, pc_range)
    voxels = dict(shape=grid, range=np.asarray(pc_range, np.float32), size=np.asarray(voxel_size, np.float32))
    targets = assigner(gt, voxels=voxels)
    ex = dict(voxels=r.voxels, coordinates=r.coordinates, num_points=r.num_points, n_voxels=r.n_pillars,
              num_voxels=r.voxel_offsets[1:] - r.voxel_offsets[:-1], shape=[[int(g) for g in grid]] * r.B, gt_boxes_and_cls=gt,
              gt_counts=preprocess.last["counts"], augment_status=status, voxel_status=r.status)
    ex.update(targets)
    return ex

