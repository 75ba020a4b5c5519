"""CenterPoint's head post-processing on the GPU: `CenterHead.predict` / `post_processing`
(det3d/models/bbox_heads/center_head.py:294-506) through dal3_center_decode and dal3_nms (include/dal3.h), from the
network's `preds_dicts` to the `prediction.pkl` dictionary tools/dist_test.py pickles and `track.py` reads.
`CenterHeadPost` is the plain route; `DoubleFlipPost` is the one for `test_cfg.double_flip` (test-time augmentation: the
batch holds every sample four times, flipped), whose un-flip, merge and decode are one pass of dal3_center_decode_flip4.

Every sample and task is decoded and suppressed on the device first (one decode enqueue per task, one NMS enqueue for all
segments, or one per task for circle NMS with its per-task radius); the kept rows are gathered once at the end, which is
the only host synchronisation. `per_class_nms` (a `pass` in the reference) is refused.
"""
import numpy as np
import torch

from . import _hip, nms

MAP_KEYS = ("hm", "reg", "height", "dim", "rot")


def _get(cfg, name, default=None):
    if isinstance(cfg, dict):
        return cfg.get(name, default)
    return getattr(cfg, name, default)


def _map(t, layout, channels, what):
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor")
    _hip.require_gpu(t, what)
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {t.dtype}")
    if t.dim() != 4:
        raise ValueError(f"{what} must be 4-D ({layout}), got {tuple(t.shape)}")
    v = t.permute(0, 2, 3, 1) if layout == "NCHW" else t      # a (B, H, W, C) view, no copy
    if channels is not None and v.shape[3] != channels:
        raise ValueError(f"{what} must have {channels} channels, got {v.shape[3]}")
    return v


def _map_struct(v):
    return _hip.Map(_hip.ptr(v), *v.stride())


class CenterHeadPost:
    """test_cfg: the head's test configuration (a dict or an object with attributes, `nms` likewise):
    post_center_limit_range, score_threshold, out_size_factor, voxel_size, pc_range, nms.nms_iou_threshold /
    nms_pre_max_size / nms_post_max_size, optionally circular_nms with min_radius per task. num_classes: classes per
    task, as CenterHead.num_classes. capacity: rows kept per (sample, task) before NMS (default: every cell, which cannot
    overflow; a smaller one saves memory and raises when a sample needs more)."""

    VIEWS = 1                                   # maps per sample

    def __init__(self, test_cfg, num_classes, capacity=None):
        if self.VIEWS == 1 and _get(test_cfg, "double_flip", False):
            raise ValueError("double_flip (test-time augmentation) merges four views per sample: use DoubleFlipPost")
        if _get(test_cfg, "per_class_nms", False):
            raise ValueError("per_class_nms is not supported (the reference's branch is a `pass`)")
        self.num_classes = [int(c) for c in num_classes]
        self.capacity = None if capacity is None else int(capacity)
        self.range = [float(v) for v in (_get(test_cfg, "post_center_limit_range") or [])]
        if len(self.range) not in (0, 6):
            raise ValueError("post_center_limit_range must be empty or hold 6 values")
        self.score_threshold = float(_get(test_cfg, "score_threshold"))
        self.out_size_factor = float(_get(test_cfg, "out_size_factor"))
        self.voxel_size = [float(v) for v in _get(test_cfg, "voxel_size")[:2]]
        self.pc_range = [float(v) for v in _get(test_cfg, "pc_range")[:2]]
        cfg_nms = _get(test_cfg, "nms")
        self.post_max = int(_get(cfg_nms, "nms_post_max_size") or 0)
        self.circular = bool(_get(test_cfg, "circular_nms", False))
        if self.circular:
            self.min_radius = [float(r) for r in _get(test_cfg, "min_radius")]
            if len(self.min_radius) < len(self.num_classes):
                raise ValueError("min_radius needs one value per task")
            self.pre_max = 0
        else:
            self.iou_threshold = float(_get(cfg_nms, "nms_iou_threshold"))
            self.pre_max = int(_get(cfg_nms, "nms_pre_max_size") or 0)

    # ------------------------------------------------------------------ device part
    def decode_nms(self, preds_dicts, layout="NCHW"):
        """decode and NMS of every (task, sample), enqueued with no sync -> a dict of device tensors: boxes (K, 9 or 7),
        scores, labels (class within the task), cell, seg_count (F), keep (F, stride), keep_count (F), status (1), and the
        host seg_offsets (F + 1); segment f = task * B + sample."""
        return self.suppress(self.decode(preds_dicts, layout))

    def decode(self, preds_dicts, layout="NCHW"):
        """the decode alone: decode_nms's dict without keep / keep_count"""
        if layout not in ("NCHW", "NHWC"):
            raise ValueError("layout must be 'NCHW' (the network's outputs) or 'NHWC' (after the reference's permute)")
        T = len(self.num_classes)
        self._samples(preds_dicts)
        tasks = []
        for t, pd in enumerate(preds_dicts):
            hm = _map(pd["hm"], layout, self.num_classes[t], f"preds_dicts[{t}]['hm']")
            maps = {"hm": hm}
            for key, ch in (("reg", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2)):
                if key == "vel" and "vel" not in pd:
                    continue
                maps[key] = _map(pd[key], layout, ch, f"preds_dicts[{t}]['{key}']")
                if maps[key].shape[:3] != hm.shape[:3] or maps[key].device != hm.device:
                    raise ValueError(f"preds_dicts[{t}]['{key}'] does not match hm's batch / size / device")
            tasks.append(maps)
        n_maps, dev = tasks[0]["hm"].shape[0], tasks[0]["hm"].device
        has_vel = "vel" in tasks[0]
        for maps in tasks:
            if maps["hm"].shape[0] != n_maps or ("vel" in maps) != has_vel or maps["hm"].device != dev:
                raise ValueError("the tasks differ in batch size, device or in having 'vel'")
        B = n_maps // self.VIEWS
        cols = 9 if has_vel else 7
        caps = []
        for maps in tasks:
            hw = maps["hm"].shape[1] * maps["hm"].shape[2]
            caps.append(hw if self.capacity is None else min(self.capacity, hw))
        off = np.zeros(T * B + 1, np.int64)
        off[1:] = np.cumsum(np.repeat(caps, B))
        F, K = T * B, int(off[-1])
        off_dev = torch.from_numpy(off).to(dev)
        boxes = torch.empty((K, cols), dtype=torch.float32, device=dev)
        scores = torch.empty(K, dtype=torch.float32, device=dev)
        labels = torch.empty(K, dtype=torch.int32, device=dev)
        cell = torch.empty(K, dtype=torch.int32, device=dev)
        seg_count = torch.zeros(F, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        lib = _hip.lib()
        for t, maps in enumerate(tasks):
            _, H, W, C = maps["hm"].shape
            if B == 0:
                break
            nbytes = self._workspace_bytes(lib, B, H, W)
            ws = _hip.workspace(nbytes, dev)
            a = _hip.CenterDecodeArgs(B=B, H=H, W=W, C=C, has_range=1 if self.range else 0, hm=_map_struct(maps["hm"]),
                                      reg=_map_struct(maps["reg"]), height=_map_struct(maps["height"]),
                                      dim=_map_struct(maps["dim"]), rot=_map_struct(maps["rot"]),
                                      vel=_map_struct(maps["vel"]) if has_vel else _hip.Map(),
                                      out_size_factor=self.out_size_factor, score_threshold=self.score_threshold, F=F, K=K,
                                      seg_first=t * B, seg_step=1, seg_offsets=_hip.ptr(off_dev), boxes=_hip.ptr(boxes),
                                      scores=_hip.ptr(scores), labels=_hip.ptr(labels), cell=_hip.ptr(cell),
                                      seg_count=_hip.ptr(seg_count), status=_hip.ptr(status), max_workgroups=0,
                                      workspace=_hip.ptr(ws), workspace_bytes=nbytes)
            a.voxel_size[:] = self.voxel_size
            a.pc_range[:] = self.pc_range
            if self.range:
                a.range[:] = self.range
            self._launch(lib, a)
        return {"boxes": boxes, "scores": scores, "labels": labels, "cell": cell, "seg_count": seg_count, "status": status,
                "seg_offsets": off, "seg_offsets_device": off_dev, "B": B}

    def _samples(self, preds_dicts):
        """the samples that come out: the maps' batch over the views per sample, checked before anything is enqueued"""
        if len(preds_dicts) != len(self.num_classes):
            raise ValueError(f"{len(preds_dicts)} prediction dicts for {len(self.num_classes)} tasks")
        hm = preds_dicts[0]["hm"]
        if not torch.is_tensor(hm):
            raise TypeError("preds_dicts[0]['hm'] must be a tensor")
        if hm.dim() != 4:
            raise ValueError(f"preds_dicts[0]['hm'] must be 4-D, got {tuple(hm.shape)}")
        if hm.shape[0] % self.VIEWS:
            raise ValueError(f"double_flip needs {self.VIEWS} views per sample: a batch of {hm.shape[0]} is no multiple of it")
        return hm.shape[0] // self.VIEWS

    @staticmethod
    def _workspace_bytes(lib, B, H, W):
        return lib.dal3_center_decode_workspace_bytes(B, H, W)

    @staticmethod
    def _launch(lib, a):
        _hip.check(lib.dal3_center_decode(a, _hip.stream()))

    def suppress(self, r):
        """the NMS of a decode() result, added to it as keep / keep_count"""
        boxes, scores, seg_count, status = r["boxes"], r["scores"], r["seg_count"], r["status"]
        off, off_dev, B, dev = r["seg_offsets"], r["seg_offsets_device"], r["B"], r["boxes"].device
        T = len(self.num_classes)
        F = T * B
        if self.circular:
            stride = nms.keep_stride(off, self.post_max)
            keep = torch.empty((F, stride), dtype=torch.int32, device=dev)
            keep_count = torch.zeros(F, dtype=torch.int32, device=dev)
            for t in range(T):
                lo, hi = int(off[t * B]), int(off[(t + 1) * B])
                if B == 0:
                    break
                k, c = nms.batched_nms(boxes[lo:hi], scores[lo:hi], off[t * B:(t + 1) * B + 1] - lo, "circle",
                                       self.min_radius[t], 0, self.post_max, seg_count=seg_count[t * B:(t + 1) * B],
                                       status=status)
                keep[t * B:(t + 1) * B, :k.shape[1]] = k
                keep_count[t * B:(t + 1) * B] = c
        else:
            keep, keep_count = nms.batched_nms(boxes, scores, off, "rotate", self.iou_threshold, self.pre_max, self.post_max,
                                               seg_count=seg_count, mirror=True, status=status,
                                               seg_offsets_device=off_dev)
        return dict(r, keep=keep, keep_count=keep_count)

    @staticmethod
    def check_status(status):
        st = int(status.item())
        if st & _hip.DECODE_OVERFLOW:
            raise RuntimeError("detect: a sample holds more cells above the threshold than the capacity per (sample, task) "
                               "(dal3_center_decode status DAL3_DECODE_OVERFLOW): raise `capacity`")
        if st & _hip.NMS_TOO_MANY:
            raise RuntimeError("detect: more NMS candidates in one segment than DAL3_NMS_MAX_PRE: set nms_pre_max_size")
        if st & _hip.NMS_BAD_SEGMENT:
            raise RuntimeError("detect: the segment table was rejected on the device (status DAL3_NMS_BAD_SEGMENT)")

    # ------------------------------------------------------------------ the reference's interface
    @torch.no_grad()
    def predict(self, preds_dicts, metadata=None, layout="NCHW"):
        """center_head.py:294: -> ret_list, per sample {'box3d_lidar' (n, 9 or 7) float32, 'scores' (n) float32,
        'label_preds' (n) int64 with the cumulative class offset of its task, 'metadata'}; tasks in order, within a task
        in keep order. preds_dicts are not modified (the reference permutes them in place)."""
        B, T = self._samples(preds_dicts), len(self.num_classes)
        if metadata is not None and self.VIEWS > 1 and B > 0 and len(metadata) == self.VIEWS * B:
            metadata = metadata[::self.VIEWS]                       # one entry per view: the sample's first (center_head.py:340)
        if metadata is not None and len(metadata) != B:
            raise ValueError(f"{len(metadata)} metadata entries for {B} samples")
        r = self.decode_nms(preds_dicts, layout)
        F = T * B
        dev = r["boxes"].device
        counts = r["keep_count"].cpu().numpy().astype(np.int64)    # the one synchronisation
        self.check_status(r["status"])
        # segments sample-major, tasks in order: one gather for everything
        perm = torch.arange(F, device=dev).reshape(T, B).t().reshape(-1)
        stride = r["keep"].shape[1]
        live = torch.arange(stride, device=dev)[None, :] < r["keep_count"][perm][:, None]
        rows = (r["keep"][perm].to(torch.int64) + r["seg_offsets_device"][:F][perm][:, None])[live]
        flag = torch.tensor(np.concatenate([[0], np.cumsum(self.num_classes)[:-1]]), dtype=torch.int64, device=dev)
        base = flag.repeat_interleave(B)[perm][:, None].expand(F, stride)[live]
        box3d, scores = r["boxes"][rows], r["scores"][rows]
        label = r["labels"][rows].to(torch.int64) + base
        per_sample = counts.reshape(T, B).sum(0)
        ends = np.cumsum(per_sample)
        ret_list = []
        for i in range(B):
            lo, hi = int(ends[i] - per_sample[i]), int(ends[i])
            ret_list.append({"box3d_lidar": box3d[lo:hi], "scores": scores[lo:hi], "label_preds": label[lo:hi],
                             "metadata": None if metadata is None else metadata[i]})
        return ret_list

    @staticmethod
    def to_prediction(ret_list):
        """tools/dist_test.py:169-178: {token: output}, every tensor on the CPU — the dictionary saved as prediction.pkl"""
        out = {}
        for output in ret_list:
            meta = output["metadata"]
            if meta is None or "token" not in meta:
                raise ValueError("to_prediction needs metadata with a 'token' for every sample")
            out[meta["token"]] = {k: (v if k == "metadata" else v.cpu()) for k, v in output.items()}
        return out


class DoubleFlipPost(CenterHeadPost):
    """CenterHeadPost for `test_cfg.double_flip` (center_head.py:318-414): `preds_dicts` hold 4 B samples, sample b's views
    at 4 b .. 4 b + 3 in the order Reformat returns them (the sweep, y = -y, x = -x, both). `decode` un-flips, merges and
    decodes them in one pass (dal3_center_decode_flip4, whose header comment is the arithmetic) into B samples; everything
    after it is CenterHeadPost's. `predict` takes the metadata of the 4 B views (every fourth is kept) or of the B samples."""

    VIEWS = 4

    @staticmethod
    def _workspace_bytes(lib, B, H, W):
        return lib.dal3_center_decode_flip4_workspace_bytes(B, H, W)

    @staticmethod
    def _launch(lib, a):
        _hip.check(lib.dal3_center_decode_flip4(_hip.CenterDecodeFlip4Args(decode=a), _hip.stream()))
