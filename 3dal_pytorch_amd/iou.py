"""Rotated-box IoU on the GPU through lib3dal_hip.so (dal3_box_iou_pairwise / dal3_box_iou_paired, include/dal3.h):
the quantity of the reference's det3d/ops/iou3d_nms/iou3d_nms_utils.py `boxes_iou_bev` / `boxes_iou3d_gpu`, under
the same names where they exist.

Boxes are (n, 7) [x, y, z, l, w, h, yaw]: z the centre, yaw about +z, l along the heading (the det3d convention the
heads emit). Inputs are CUDA tensors, float32 or float64; outputs are float32 on the same device, computed on the
current stream. A union <= 0 gives 0, a non-finite input NaN for its pairs.
"""
import torch

from . import _hip

_F64 = {torch.float32: 0, torch.float64: 1}


def _boxes(t, what):
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor")
    _hip.require_gpu(t, what)
    if t.dim() != 2 or t.shape[1] != 7:
        raise ValueError(f"{what} must be (n, 7) [x, y, z, l, w, h, yaw], got {tuple(t.shape)}")
    if t.dtype not in _F64:
        raise TypeError(f"{what} must be float32 or float64, got {t.dtype}")
    return t.contiguous()


def _pairwise(a, b, bev, v3):
    a, b = _boxes(a, "boxes_a"), _boxes(b, "boxes_b")
    if a.dtype != b.dtype:
        raise TypeError(f"boxes_a and boxes_b differ in dtype ({a.dtype} vs {b.dtype})")
    n, m = a.shape[0], b.shape[0]
    out_bev = torch.empty((n, m), dtype=torch.float32, device=a.device) if bev else None
    out_3d = torch.empty((n, m), dtype=torch.float32, device=a.device) if v3 else None
    if n and m:
        _hip.check(_hip.lib().dal3_box_iou_pairwise(_hip.ptr(a), n, _hip.ptr(b), m, _F64[a.dtype], _hip.ptr(out_bev),
                                                    _hip.ptr(out_3d), _hip.stream()))
    return out_bev, out_3d


def boxes_iou_bev(boxes_a, boxes_b):
    """(n, 7) x (m, 7) -> (n, m) float32 bird's-eye-view IoU"""
    return _pairwise(boxes_a, boxes_b, True, False)[0]


def boxes_iou3d(boxes_a, boxes_b):
    """(n, 7) x (m, 7) -> (n, m) float32 3D IoU: BEV overlap x z overlap over the union of the volumes"""
    return _pairwise(boxes_a, boxes_b, False, True)[1]


def boxes_iou_bev_3d(boxes_a, boxes_b):
    """(n, 7) x (m, 7) -> ((n, m) BEV IoU, (n, m) 3D IoU) from one launch"""
    return _pairwise(boxes_a, boxes_b, True, True)


def paired_iou(boxes_a, boxes_b):
    """(n, 7) vs (n, 7), row k against row k -> (iou_bev (n,), iou_3d (n,)) float32, one launch"""
    a, b = _boxes(boxes_a, "boxes_a"), _boxes(boxes_b, "boxes_b")
    if a.dtype != b.dtype:
        raise TypeError(f"boxes_a and boxes_b differ in dtype ({a.dtype} vs {b.dtype})")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"paired_iou needs as many boxes on both sides ({a.shape[0]} vs {b.shape[0]})")
    n = a.shape[0]
    out_bev = torch.empty(n, dtype=torch.float32, device=a.device)
    out_3d = torch.empty(n, dtype=torch.float32, device=a.device)
    if n:
        _hip.check(_hip.lib().dal3_box_iou_paired(_hip.ptr(a), _hip.ptr(b), n, _F64[a.dtype], _hip.ptr(out_bev),
                                                  _hip.ptr(out_3d), _hip.stream()))
    return out_bev, out_3d
