"""The detection run's input: the Waymo val data set on the host and the sweep merge on the device.

`WaymoDataset` is det3d/datasets/waymo/waymo.py under the reference's name and arguments for the val / test / `mytrain`
use: the infos file, `load_interval`, `_num_point_features`, and the config's pipeline READ (its entries checked, the
voxel generator's numbers taken), not executed. `merge_sweeps` is the WaymoDataset branch of LoadPointCloudFromFile
(det3d/datasets/pipelines/loading.py:61-91, 140-168) through dal3_sweep_merge (include/dal3.h has the arithmetic): the
frame files' raw `points_xyz` and `points_feature` stay in planes of their own, nothing is concatenated on the host and no
`tanh` runs there. `SweepLoader` feeds it: every frame file is staged in pinned memory by a background thread, uploaded
once on a copy stream into a small least-recently-used arena keyed by the file's path (frame t is sweep 0 of frame t + 1,
so a sequence-ordered run uploads each file once, not nsweeps times) and merged a batch at a time on the current stream,
ordered by events. Nothing here synchronises the host with the device.
"""
import collections
import pickle
import threading

import numpy as np
import torch

from . import _hip
from .eval import reorganize_info  # noqa: F401  (tools/utils.py:46-51: the run and its callers take it from here)

PIPELINE_READ = ("LoadPointCloudFromFile", "LoadPointCloudAnnotations", "Preprocess", "Voxelization", "AssignLabel", "Reformat")
# dal3_sweep_segment as a NumPy record (checked against the ctypes mirror below): a batch's table is filled by columns
SEGMENT = np.dtype([("xyz", "<u8"), ("feature", "<u8"), ("n", "<i8"), ("out_row", "<i8"), ("matrix", "<f8", (12,)),
                    ("time", "<f4"), ("has_transform", "<i4")])
assert SEGMENT.itemsize == _hip.C.sizeof(_hip.SweepSegment)


def _get(cfg, key, default=None):
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


class WaymoDataset:
    """det3d/datasets/waymo/waymo.py for inference. `pipeline`: the config's list of dicts, read: every entry must be one of
    PIPELINE_READ; Preprocess must say mode="val" and shuffle_points=False (the val pass-through, preprocess.py: nothing is
    done to the points); Voxelization's cfg gives `voxel_generator` = {range, voxel_size, max_points_in_voxel,
    max_voxel_num}, and `max_voxels` is the val capacity, the second entry of max_voxel_num (preprocess.py:191-193)."""
    NumPointFeatures = 5                                    # x, y, z, intensity, elongation

    def __init__(self, info_path, root_path, nsweeps=1, load_interval=1, test_mode=True, class_names=None, pipeline=None, **kw):
        if not test_mode:
            raise NotImplementedError("WaymoDataset(test_mode=False): the training pipeline (GT paste, augmentation, shuffle) "
                                      "is not a data set here: the detectors' train_step_from_sweeps takes resident sweeps")
        self.load_interval, self.nsweeps, self.test_mode = int(load_interval), int(nsweeps), True
        if not 1 <= self.nsweeps <= _hip.SWEEP_MAX:
            raise ValueError(f"nsweeps = {nsweeps}: 1 .. {_hip.SWEEP_MAX}")
        print("Using {} sweeps".format(nsweeps))
        self._info_path, self._root_path, self._class_names = info_path, root_path, class_names
        self._num_point_features = self.NumPointFeatures if self.nsweeps == 1 else self.NumPointFeatures + 1
        self.voxel_generator = None
        self.pipeline = self._read_pipeline(pipeline)

    @staticmethod
    def _refuse(what):
        raise ValueError(f"WaymoDataset: {what}")

    def _read_pipeline(self, pipeline):
        steps = [] if pipeline is None else list(pipeline)
        for step in steps:
            kind = _get(step, "type")
            if kind not in PIPELINE_READ:
                self._refuse(f"pipeline step {kind!r} is not read here (known: {', '.join(PIPELINE_READ)})")
            cfg = _get(step, "cfg")
            if kind == "LoadPointCloudFromFile" and _get(step, "dataset", "WaymoDataset") != "WaymoDataset":
                self._refuse(f"LoadPointCloudFromFile(dataset={_get(step, 'dataset')!r}): only the WaymoDataset branch is built")
            if kind == "Preprocess":
                mode, shuffle = _get(cfg, "mode"), _get(cfg, "shuffle_points", False)
                if mode != "val":
                    self._refuse(f"Preprocess(mode={mode!r}) is refused: this data set is the inference input, whose Preprocess "
                                 "is the val pass-through (mode=\"val\"); the training augmentation is augment.Preprocess")
                if shuffle:
                    self._refuse("Preprocess(shuffle_points=True) is refused: the val pass-through keeps the points in file "
                                 "order (a shuffle would change which points a full voxel keeps)")
            if kind == "Voxelization":
                num = _get(cfg, "max_voxel_num")
                num = [num, num] if isinstance(num, int) else list(num)
                self.voxel_generator = dict(range=list(_get(cfg, "range")), voxel_size=list(_get(cfg, "voxel_size")),
                                            max_points_in_voxel=int(_get(cfg, "max_points_in_voxel")),
                                            max_voxel_num=num, max_voxels=int(num[1]))
        return steps

    def load_infos(self, info_path):
        with open(self._info_path, "rb") as f:
            _waymo_infos_all = pickle.load(f)
        self._waymo_infos = _waymo_infos_all[::self.load_interval]
        print("Using {} Frames".format(len(self._waymo_infos)))

    def __len__(self):
        if not hasattr(self, "_waymo_infos"):
            self.load_infos(self._info_path)
        return len(self._waymo_infos)

    def info(self, idx):
        len(self)
        return self._waymo_infos[idx]

    def metadata(self, idx):
        """get_sensor_data's `metadata` (waymo.py:76-80), which Reformat hands on unchanged"""
        return {"image_prefix": self._root_path, "num_point_features": self._num_point_features, "token": self.info(idx)["token"]}

    def sweeps(self, idx):
        """the sample's segments in merge order: [(path, transform_matrix | None, time_lag)], the current frame first"""
        info = self.info(idx)
        out = [(info["path"], None, 0.0)]
        if self.nsweeps > 1:
            assert (self.nsweeps - 1) == len(info["sweeps"]), "nsweeps {} should be equal to the list length {}.".format(
                self.nsweeps, len(info["sweeps"]))
            for i in range(self.nsweeps - 1):
                sweep = info["sweeps"][i]
                out.append((sweep["path"], sweep["transform_matrix"], sweep["time_lag"]))
        return out

    def __getitem__(self, idx):
        return {"metadata": self.metadata(idx), "sweeps": self.sweeps(idx), "mode": "val", "type": "WaymoDataset"}


# ------------------------------------------------------------------------------------------- the merge
def _plane(t, cols, what, dev):
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor")
    _hip.require_gpu(t, what)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != cols or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 (n, {cols}) tensor, got {t.dtype} {tuple(t.shape)}")
    if dev is not None and t.device != dev:
        raise ValueError(f"{what} lives on {t.device}, the other planes on {dev}")
    return t


def segment_table(samples, nsweeps):
    """samples: per sample its nsweeps segments (xyz (n, 3), feature (n, 2), transform_matrix (4, 4) | None, time_lag), CUDA
    float32 planes -> (table, a SEGMENT record array on the host; point_offsets (B + 1) int64; device)"""
    nsweeps = int(nsweeps)
    if not 1 <= nsweeps <= _hip.SWEEP_MAX:
        raise ValueError(f"nsweeps = {nsweeps}: 1 .. {_hip.SWEEP_MAX}")
    table = np.zeros(len(samples) * nsweeps, SEGMENT)
    dev, row, s = None, 0, 0
    offsets = np.zeros(len(samples) + 1, np.int64)
    for b, sample in enumerate(samples):
        if len(sample) != nsweeps:
            raise ValueError(f"sample {b} has {len(sample)} segments, nsweeps is {nsweeps}")
        for k, (xyz, feature, matrix, time_lag) in enumerate(sample):
            xyz = _plane(xyz, 3, f"sample {b} sweep {k}: xyz", dev)
            dev = xyz.device
            feature = _plane(feature, 2, f"sample {b} sweep {k}: feature", dev)
            if feature.shape[0] != xyz.shape[0]:
                raise ValueError(f"sample {b} sweep {k}: {xyz.shape[0]} xyz rows, {feature.shape[0]} feature rows")
            e = table[s]
            e["xyz"], e["feature"], e["n"], e["out_row"] = xyz.data_ptr(), feature.data_ptr(), xyz.shape[0], row
            if k == 0 and (matrix is not None or time_lag):
                raise ValueError(f"sample {b}: the current frame takes no transform and no time_lag")
            if matrix is not None:
                m = np.asarray(matrix, np.float64)
                if m.shape != (4, 4):
                    raise ValueError(f"sample {b} sweep {k}: transform_matrix must be (4, 4), got {m.shape}")
                e["matrix"], e["has_transform"] = m[:3].reshape(12), 1
            e["time"] = np.float32(time_lag)
            row += xyz.shape[0]
            s += 1
        offsets[b + 1] = row
    return table, offsets, dev


def merge_sweeps(samples, nsweeps, *, max_workgroups=0, out=None, point_offsets_device=None):
    """LoadPointCloudFromFile's Waymo merge of a batch in one enqueue (dal3_sweep_merge). samples: see segment_table ->
    (points (N, 5 | 6) float32, point_offsets (B + 1) int64 on the host, point_offsets_device): what detect takes. The
    table goes up from pinned memory without blocking; no synchronisation. out / point_offsets_device: buffers to write."""
    table, offsets, dev = segment_table(samples, nsweeps)
    B, N, cols = len(samples), int(offsets[-1]), 5 if int(nsweeps) == 1 else 6
    if dev is None:
        raise ValueError("merge_sweeps needs at least one sample: the device comes from its planes")
    if out is None:
        out = torch.empty((N, cols), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (N, cols) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous float32 ({N}, {cols}) tensor on {dev}")
    if point_offsets_device is None:
        point_offsets_device = torch.empty(B + 1, dtype=torch.int64, device=dev)
    elif point_offsets_device.dtype != torch.int64 or point_offsets_device.numel() != B + 1 or point_offsets_device.device != dev:
        raise ValueError(f"point_offsets_device must be an int64 ({B + 1}) tensor on {dev}")
    staged = torch.empty(table.nbytes, dtype=torch.uint8, pin_memory=True)
    staged.numpy()[:] = table.view(np.uint8)
    table_dev = staged.to(dev, non_blocking=True)
    _hip.check(_hip.lib().dal3_sweep_merge(_hip.ptr(table_dev), B, int(nsweeps), N, _hip.ptr(out), _hip.ptr(point_offsets_device),
                                           int(max_workgroups), _hip.stream()))
    return out, offsets, point_offsets_device


# ------------------------------------------------------------------------------------------- the loader
def read_frame(path):
    """a frame file's raw rows -> (xyz (n, 3), feature (n, 2)) float32 in pinned memory, each copied on its own"""
    with open(path, "rb") as f:
        lidars = pickle.load(f)["lidars"]
    planes = []
    for key, cols in (("points_xyz", 3), ("points_feature", 2)):
        a = np.asarray(lidars[key], np.float32).reshape(-1, cols)
        pinned = torch.empty(a.shape, dtype=torch.float32, pin_memory=True)
        pinned.numpy()[...] = a
        planes.append(pinned)
    if planes[0].shape[0] != planes[1].shape[0]:
        raise ValueError(f"{path}: {planes[0].shape[0]} points_xyz rows, {planes[1].shape[0]} points_feature rows")
    return tuple(planes)


class SweepLoader:
    """Iterates (points, point_offsets, point_offsets_device, metadata) per batch of `dataset` in its order; the last batch
    is short. capacity: the arena's frames (default batch_size + nsweeps); an evicted file is read again. `uploads`
    counts the frame files uploaded so far (a file is read exactly as often as it is uploaded: one counter).

    Batch k + 1's missing files are read and staged by a background thread while the caller works on batch k. Uploads go
    on `copy_stream`: it waits for an event of the current stream before it writes a fresh buffer (whose memory the
    current stream may still be using under an earlier name), and the current stream waits for the upload's event before
    the merge. Both planes are allocated on the current stream, so memory that the arena lets go of is reused only behind
    the kernels that read it."""

    def __init__(self, dataset, batch_size, device, capacity=None):
        self.dataset, self.batch_size, self.device = dataset, int(batch_size), torch.device(device)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.capacity = self.batch_size + dataset.nsweeps if capacity is None else int(capacity)
        if self.capacity < 1:
            raise ValueError("capacity must be >= 1 frame")
        self.arena = collections.OrderedDict()              # path -> (xyz, feature) on the device, least recent first
        self.copy_stream = torch.cuda.Stream(self.device)
        self.uploads = 0

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def _batch(self, k):
        lo = k * self.batch_size
        return list(range(lo, min(lo + self.batch_size, len(self.dataset))))

    def _missing(self, k):
        """the files batch k needs and the arena lacks, each once, in first use order"""
        paths = []
        for idx in self._batch(k):
            for path, _, _ in self.dataset.sweeps(idx):
                if path not in self.arena and path not in paths:
                    paths.append(path)
        return paths

    def _stage(self, k):
        """start reading batch k's missing files -> (thread, its result box)"""
        box = {}

        def work(paths=self._missing(k)):
            try:
                box["frames"] = {p: read_frame(p) for p in paths}
            except BaseException as e:                      # handed to the consumer, which raises it
                box["error"] = e
        t = threading.Thread(target=work, name="sweep-stage", daemon=True)
        t.start()
        return t, box

    def _upload(self, staged):
        """staged frames -> device planes, on the copy stream; -> {path: (xyz, feature)}"""
        if not staged:
            return {}
        cur = torch.cuda.current_stream(self.device)
        planes = {p: tuple(torch.empty(h.shape, dtype=torch.float32, device=self.device) for h in host)
                  for p, host in staged.items()}
        self.copy_stream.wait_event(cur.record_event())
        with torch.cuda.stream(self.copy_stream):
            for p, host in staged.items():
                for dst, src in zip(planes[p], host):
                    dst.copy_(src, non_blocking=True)
            done = self.copy_stream.record_event()
        cur.wait_event(done)
        self.uploads += len(staged)
        return planes

    def __iter__(self):
        n = len(self)
        if n == 0:
            return
        job = self._stage(0)
        with torch.cuda.device(self.device):
            for k in range(n):
                thread, box = job
                thread.join()
                if "error" in box:
                    raise box["error"]
                # this batch's planes, held whatever the arena lets go of meanwhile: the fresh ones and, of the arena's, those
                # that the plan counted on (the arena has not changed since _stage(k) looked)
                held = self._upload(box["frames"])
                for idx in self._batch(k):
                    for path, _, _ in self.dataset.sweeps(idx):
                        if path not in held:
                            held[path] = self.arena[path]
                samples, metadata = [], []
                for idx in self._batch(k):
                    sample = []
                    for path, matrix, time_lag in self.dataset.sweeps(idx):
                        self.arena[path] = held[path]
                        self.arena.move_to_end(path)
                        while len(self.arena) > self.capacity:
                            self.arena.popitem(last=False)
                        sample.append(held[path] + (matrix, time_lag))
                    samples.append(sample)
                    metadata.append(self.dataset.metadata(idx))
                if k + 1 < n:
                    job = self._stage(k + 1)
                points, offsets, offsets_dev = merge_sweeps(samples, self.dataset.nsweeps)
                yield points, offsets, offsets_dev, metadata
