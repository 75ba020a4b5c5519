"""Non-maximum suppression on the GPU through lib3dal_hip.so (dal3_nms, include/dal3.h), under the reference's names and
signatures: `rotate_nms_pcdet` (det3d/core/bbox/box_torch_ops.py:248), `nms_gpu`
(det3d/ops/iou3d_nms/iou3d_nms_utils.py:75) and `circle_nms` (det3d/models/bbox_heads/center_head.py:498, there
`_circle_nms`), plus `batched_nms`: many (frame, task) segments in one enqueue with no host round trip.

Boxes are float32 or float64 CUDA tensors [x, y, z, l, w, h, ..., yaw], taken as iou.py takes them (column 3 along the
yaw): what the reference's `nms_gpu` is handed. `rotate_nms_pcdet` converts ITS boxes first, as the reference's does
(columns 3 / 4 swapped, yaw -> -yaw - pi/2): that changes the IoUs (the centres stay, the rectangles turn), so it is
applied, inside the kernel as each box is loaded (`mirror=True`), without a copy. The result is defined exactly
(include/dal3.h): candidates by score descending, NaN first, EQUAL SCORES BY ASCENDING ROW (the reference's sorts are not
stable there), the first pre_max of them; greedy scan with `iou_bev > thresh` (the bits of iou.boxes_iou_bev) or, for
circles, `dx*dx + dy*dy <= thresh`; the first post_max kept.
"""
import numpy as np
import torch

from . import _hip

_F64 = {torch.float32: 0, torch.float64: 1}
MODES = {"rotate": _hip.NMS_ROTATE, "circle": _hip.NMS_CIRCLE}


def _boxes(t, what):
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor")
    _hip.require_gpu(t, what)
    if t.dim() != 2 or t.shape[1] < 7:
        raise ValueError(f"{what} must be (n, 7 or more) [x, y, z, l, w, h, ..., yaw], got {tuple(t.shape)}")
    if t.dtype not in _F64:
        raise TypeError(f"{what} must be float32 or float64, got {t.dtype}")
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def _scores(t, n, device):
    if not torch.is_tensor(t):
        raise TypeError("scores must be a tensor")
    _hip.require_gpu(t, "scores")
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError(f"scores must be ({n},) like the boxes, got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"scores live on {t.device}, the boxes on {device}")
    return t.to(torch.float32).contiguous()


def keep_stride(seg_offsets, post_max):
    """the row length batched_nms gives `keep`: min(post_max or N, N), N the largest segment"""
    off = np.asarray(seg_offsets, dtype=np.int64).reshape(-1)
    n = int(np.diff(off).max()) if off.size > 1 else 0
    return min(int(post_max), n) if post_max else n


def batched_nms(boxes, scores, seg_offsets, mode, thresh, pre_max=0, post_max=0, *, seg_count=None, yaw_col=-1,
                mirror=False, status=None, max_workgroups=0, seg_offsets_device=None, return_order=False):
    """NMS of F segments in one enqueue, no sync. boxes (K, >= 7), scores (K): segment f = rows
    [seg_offsets[f], seg_offsets[f + 1]) (the first seg_count[f] of them with `seg_count`, a device int32 tensor).
    seg_offsets lives on the HOST. mode 'rotate' / 'circle'; pre_max / post_max 0 or None: no cut. yaw_col: the yaw's
    column (-1: the last, center_head.py:471's [0, 1, 2, 3, 4, 5, -1] without a copy). mirror: convert every box as
    rotate_nms_pcdet does before it is used (module docstring).

    -> (keep (F, stride) int32: rows relative to the segment, keep_count (F) int32), device tensors; entries of a row
    beyond its count are undefined. status: a device int32 (1) the kernels OR problems into (_hip.NMS_*); without one, a
    segment that could exceed dal3's candidate bound is refused here.
    """
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    boxes = _boxes(boxes, "boxes")
    K, cols = boxes.shape
    scores = _scores(scores, K, boxes.device)
    off = _hip.host_offsets(seg_offsets, K, "seg_offsets", "the sizes of the outputs come", "F")
    F = off.size - 1
    pre_max, post_max = int(pre_max or 0), int(post_max or 0)
    if pre_max < 0 or post_max < 0:
        raise ValueError("pre_max / post_max must be >= 0")
    if pre_max > _hip.NMS_MAX_PRE:
        raise ValueError(f"pre_max {pre_max} is above the bound on candidates per segment ({_hip.NMS_MAX_PRE})")
    yaw = yaw_col if yaw_col >= 0 else cols + yaw_col
    if not 6 <= yaw < cols:
        raise ValueError(f"yaw_col {yaw_col} is not a column from 6 on of {cols}-column boxes")
    biggest = int(np.diff(off).max()) if F else 0
    if status is None and pre_max == 0 and biggest > _hip.NMS_MAX_PRE:
        raise ValueError(f"a segment of {biggest} rows exceeds the {_hip.NMS_MAX_PRE} candidates one segment may have: give "
                         "pre_max, or a status tensor to have it reported on the device")
    dev = boxes.device
    stride = keep_stride(off, post_max)
    keep = torch.empty((F, stride), dtype=torch.int32, device=dev)
    count = torch.zeros(F, dtype=torch.int32, device=dev)
    order = torch.empty(K, dtype=torch.int32, device=dev) if return_order else None
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    if seg_count is not None:
        _hip.require_gpu(seg_count, "seg_count")
        if seg_count.dtype != torch.int32 or seg_count.shape != (F,) or not seg_count.is_contiguous():
            raise ValueError(f"seg_count must be a contiguous int32 ({F},) tensor")
    if F:
        off_dev = seg_offsets_device if seg_offsets_device is not None else torch.from_numpy(off).to(dev)
        lib = _hip.lib()
        nbytes = lib.dal3_nms_workspace_bytes(K, _F64[boxes.dtype])
        ws = _hip.workspace(nbytes, dev)
        a = _hip.NmsArgs(F=F, K=K, seg_offsets=_hip.ptr(off_dev), seg_offsets_host=off.ctypes.data, seg_count=_hip.ptr(seg_count),
                         boxes=_hip.ptr(boxes), scores=_hip.ptr(scores), box_stride=boxes.stride(0) if K else cols, yaw_col=yaw,
                         boxes_f64=_F64[boxes.dtype], mode=MODES[mode], thresh=float(thresh), pre_max=pre_max,
                         post_max=post_max, stride=stride, max_workgroups=int(max_workgroups), mirror=1 if mirror else 0, keep=_hip.ptr(keep),
                         keep_count=_hip.ptr(count), order=_hip.ptr(order), status=_hip.ptr(status), workspace=_hip.ptr(ws),
                         workspace_bytes=nbytes)
        _hip.check(lib.dal3_nms(a, _hip.stream()))
    return (keep, count, order) if return_order else (keep, count)


def _single(boxes, scores, mode, thresh, pre_max, post_max, mirror=False):
    n = boxes.shape[0]
    if pre_max is not None and int(pre_max) >= n:
        pre_max = 0                                         # a cut at or above n is no cut
    keep, count = batched_nms(boxes, scores, [0, n], mode, thresh, pre_max, post_max, mirror=mirror)
    return keep[0, :int(count.item())].to(torch.int64)


def rotate_nms_pcdet(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    """box_torch_ops.py:248: boxes (N, 7) [x, y, z, l, w, h, theta], scores (N) -> LongTensor of kept rows, best first"""
    return _single(boxes, scores, "rotate", thresh, pre_maxsize, post_max_size, mirror=True)


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """iou3d_nms_utils.py:75: boxes (N, 7) [x, y, z, dx, dy, dz, heading] -> (LongTensor of kept rows, None)"""
    if boxes.shape[1] != 7:
        raise ValueError(f"boxes must be (n, 7), got {tuple(boxes.shape)}")
    return _single(boxes, scores, "rotate", thresh, pre_maxsize, None), None


def circle_nms(boxes_xy_score, min_radius, post_max_size=83):
    """center_head.py:498: boxes (N, 3) [x, y, score] -> LongTensor of kept rows; a box within sqrt(min_radius) of a kept
    one (the squared distance is compared with min_radius itself, as circle_nms_jit does) is suppressed"""
    t = boxes_xy_score
    if not torch.is_tensor(t):
        raise TypeError("boxes must be a tensor")
    _hip.require_gpu(t, "boxes")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"boxes must be (n, 3) [x, y, score], got {tuple(t.shape)}")
    if t.dtype not in _F64:
        raise TypeError(f"boxes must be float32 or float64, got {t.dtype}")
    b = torch.zeros((t.shape[0], 7), dtype=t.dtype, device=t.device)
    b[:, :2] = t[:, :2]
    return _single(b, t[:, 2], "circle", min_radius, None, post_max_size)
