"""Box-estimation metrics of the training run on the GPU through lib3dal_hip.so (dal3_box_estimation_metrics,
include/dal3.h): the numbers static_train.py / dynamic_train.py and their eval_one_epoch compute per step with
compute_box3d_iou (tools/utils.py:81-103) on the host — decode of both boxes (argmax class + residual, in float64),
BEV / 3D IoU of the pair, the box estimation accuracy at IoU 0.7 and the segmentation accuracy — in one launch per
batch, accumulated on the device with no host sync.

The IoU of a pair is the rotated-box IoU of iou.py (float64 boxes): the same substitution as eval.box_metrics, for the
un-vendored fpointnet_train.provider_fpointnet geometry. Per item it is the bits of
iou.paired_iou(pred, label) on the float64 boxes the decode gives.

Every per-item field is passed as it comes out of the model — most are column slices of the (B, 39) box_pred — and
read through its row stride, with no copy.
"""
import numpy as np
import torch

from . import _hip, arch

NUM_POINT_STATIC = 4096                 # static_train.py:21
NUM_POINT_DYNAMIC = 1024                # dynamic_train.py:21
NUM_FRAME = 5                           # dynamic_train.py:22
IOU3D_THRESHOLD = 0.7                   # static_train.py:125

_PRED = (("center", 3, 1), ("heading_scores", 12, 2), ("heading_residuals", 12, 4), ("size_scores", 3, 8),
         ("size_residuals", 9, 16))
_LABEL = (("center_label", 3, 32), ("heading_class_label", 1, 0), ("heading_residual_label", 1, 64),
          ("size_class_label", 1, 0), ("size_residual_label", 3, 128))
_I32_BIT = {"heading_class_label": 1, "size_class_label": 2}


def decode_boxes_numpy(center, heading_scores, heading_residuals, size_scores, size_residuals, center_label,
                       heading_class_label, heading_residual_label, size_class_label, size_residual_label):
    """The host statement of the kernel's decode: the two [x, y, z, l, w, h, yaw] float64 boxes per item that
    compute_box3d_iou hands to its geometry (class2angle / class2size of np.argmax classes). An out-of-range class
    label gives NaN in the values it selects. Returns (pred (B,7), label (B,7))."""
    mean = np.asarray(arch.MEAN_SIZE, np.float64)
    per = 2 * np.pi / float(arch.NUM_HEADING_BIN)

    def box(c, hc, hr, sc, sr):
        ok_h = (hc >= 0) & (hc < arch.NUM_HEADING_BIN)
        ok_s = (sc >= 0) & (sc < arch.NUM_SIZE_CLUSTER)
        a = np.where(ok_h, np.where(ok_h, hc, 0).astype(np.int64) * per + hr, np.nan)
        a = np.where(a > np.pi, a - 2 * np.pi, a)
        size = np.where(ok_s[:, None], mean[np.where(ok_s, sc, 0)] + sr, np.nan)
        return np.concatenate([np.asarray(c).astype(np.float64), size, a[:, None]], 1)
    hs, ss = np.asarray(heading_scores), np.asarray(size_scores)
    B = hs.shape[0]
    ar = np.arange(B)
    hc, sc = np.argmax(hs, 1), np.argmax(ss, 1)
    pred = box(center, hc, np.asarray(heading_residuals)[ar, hc], sc, np.asarray(size_residuals)[ar, sc, :])
    hcl, scl = np.asarray(heading_class_label).astype(np.int64), np.asarray(size_class_label).astype(np.int64)
    srl = np.asarray(size_residual_label)
    label = box(center_label, hcl, np.asarray(heading_residual_label), scl, srl)
    return pred, label


def _rows(t, name, B, width):
    """a (B, ...) device tensor whose rows hold `width` values -> (tensor, row stride in elements). A view whose rows are
    contiguous (every field the heads emit) is used in place; anything else is copied."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    _hip.require_gpu(t, name)
    if t.dim() == 0 or t.shape[0] != B or (B and t[0].numel() != width):
        raise ValueError(f"{name}: expected {B} rows of {width} value(s), got {tuple(t.shape)}")
    expect, ok = 1, True
    for d in range(t.dim() - 1, 0, -1):
        if t.shape[d] != 1 and t.stride(d) != expect:
            ok = False
        expect *= t.shape[d]
    if not ok:
        t = t.contiguous()
    return t, t.stride(0)


def _float(t, name):
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{name} must be float32 or float64, got {t.dtype}")
    return t


def _int(t, name):
    if t.dtype in (torch.int64, torch.int32):
        return t
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError(f"{name} must be an integer tensor, got {t.dtype}")
    return t.long()


def _label_fields(output, labels, two_stage):
    """the label side as compute_box3d_iou gets it: for two_box_est the stage-two heading labels the model emits"""
    lab = {"center_label": labels["center_label"], "size_class_label": labels["size_class_label"],
           "size_residual_label": labels["size_residual_label"]}
    if two_stage:
        lab["heading_class_label"] = output["heading_class_label_two"]
        lab["heading_residual_label"] = output["heading_residuals_label_two"]
    else:
        lab["heading_class_label"] = labels["heading_class_label"]
        lab["heading_residual_label"] = labels.get("heading_residuals_label", labels.get("heading_residual_label"))
    return lab


def _args(pred, lab, thr=IOU3D_THRESHOLD):
    """dal3_box_metric_args for the ten per-item fields; returns (args, tensors to keep alive)"""
    B = int(pred["center"].shape[0])
    a = _hip.BoxMetricArgs()
    a.B, a.thr = B, float(thr)
    keep = []
    for src, spec in ((pred, _PRED), (lab, _LABEL)):
        for name, width, f64_bit in spec:
            t = src[name].detach()
            if name in _I32_BIT:
                t = _int(t, name)
                if t.dtype == torch.int32:
                    a.i32_fields |= _I32_BIT[name]
            else:
                t = _float(t, name)
                if t.dtype == torch.float64:
                    a.f64_fields |= f64_bit
            t, ld = _rows(t, name, B, width)
            keep.append(t)
            setattr(a, name, _hip.ptr(t))
            setattr(a, "ld_" + name, ld)
    return a, keep


def _segmentation(a, logits, mask_label, keep):
    logits, mask_label = logits.detach(), mask_label.detach()
    _hip.require_gpu(logits, "logits")
    _hip.require_gpu(mask_label, "mask_label")
    if logits.dim() != 3 or logits.shape[2] != 2 or logits.shape[0] != a.B:
        raise ValueError(f"logits must be (B, N, 2) with B = {a.B}, got {tuple(logits.shape)}")
    if logits.dtype != torch.float32:
        raise TypeError(f"logits must be float32, got {logits.dtype}")
    if tuple(mask_label.shape) != tuple(logits.shape[:2]):
        raise ValueError(f"mask_label must be {tuple(logits.shape[:2])}, got {tuple(mask_label.shape)}")
    if mask_label.dtype in (torch.uint8, torch.bool):
        a.mask_dtype = _hip.MASK_U8
    elif mask_label.dtype == torch.float32:
        a.mask_dtype = _hip.MASK_F32
    else:
        raise TypeError(f"mask_label must be uint8, bool or float32, got {mask_label.dtype}")
    a.N = int(logits.shape[1])
    a.logits, a.mask_label = _hip.ptr(logits), _hip.ptr(mask_label)
    a.logits_stride_b, a.logits_stride_n, a.logits_stride_c = logits.stride()
    a.mask_stride_b, a.mask_stride_n = mask_label.stride()
    keep += [logits, mask_label]


def _launch(a):
    _hip.check(_hip.lib().dal3_box_estimation_metrics(a, _hip.stream()))


def box_estimation_iou(output, labels, two_stage=False):
    """(iou_bev (B,), iou_3d (B,)) float32 on the device, one launch: compute_box3d_iou on the heads' raw outputs.
    output: the model's dict (center, heading_scores, heading_residuals, size_scores, size_residuals and, for
    two_stage, heading_class_label_two / heading_residuals_label_two); labels: prep's label dict."""
    a, keep = _args(output, _label_fields(output, labels, two_stage))
    dev = output["center"].device
    vb = torch.empty(a.B, dtype=torch.float32, device=dev)
    v3 = torch.empty(a.B, dtype=torch.float32, device=dev)
    a.iou_bev, a.iou_3d = _hip.ptr(vb), _hip.ptr(v3)
    if a.B:
        _launch(a)
    return vb, v3


def compute_box3d_iou(center_pred, heading_logits, heading_residuals, size_logits, size_residuals, center_label,
                      heading_class_label, heading_residual_label, size_class_label, size_residual_label, device="cuda"):
    """tools/utils.py:81-103 with the host-array signature: (iou2d (B,), iou3d (B,)) float32 NumPy arrays. Uploads the
    ten arrays, one launch, one download."""
    dev = torch.device(device)

    def up(x, what):
        x = np.asarray(x)
        if x.dtype.kind == "f" and x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float32)
        elif x.dtype.kind in "iub" and what in _I32_BIT:
            x = x.astype(np.int64) if x.dtype != np.int32 else x
        elif x.dtype.kind in "iub":
            x = x.astype(np.float64)
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    pred = {"center": up(center_pred, "center"), "heading_scores": up(heading_logits, "heading_scores"),
            "heading_residuals": up(heading_residuals, "heading_residuals"), "size_scores": up(size_logits, "size_scores"),
            "size_residuals": up(size_residuals, "size_residuals")}
    lab = {"center_label": up(center_label, "center_label"),
           "heading_class_label": up(heading_class_label, "heading_class_label"),
           "heading_residual_label": up(heading_residual_label, "heading_residual_label"),
           "size_class_label": up(size_class_label, "size_class_label"),
           "size_residual_label": up(size_residual_label, "size_residual_label")}
    a, keep = _args(pred, lab)
    vb = torch.empty(a.B, dtype=torch.float32, device=dev)
    v3 = torch.empty(a.B, dtype=torch.float32, device=dev)
    a.iou_bev, a.iou_3d = _hip.ptr(vb), _hip.ptr(v3)
    if a.B:
        with torch.cuda.device(dev):
            _launch(a)
    return vb.cpu().numpy(), v3.cpu().numpy()


class TrainMetrics:
    """The per-epoch accumulation of static_train.py:84-135 / static_eval.py:184-209 (and the dynamic ones) on the
    device. update() is one launch per step and reads nothing back; result() reads the accumulator once.

    n_points: points per item of the segmentation accuracy's denominator (NUM_POINT, or NUM_POINT * NUM_FRAME for the
    dynamic head)."""

    def __init__(self, device, n_points, thr=IOU3D_THRESHOLD):
        self.device = torch.device(device)
        self.n_points = int(n_points)
        self.thr = float(thr)
        # dal3_box_metric_acc: 3 float64 sums then 3 uint64 counts, held as 6 int64 words
        self.acc = torch.zeros(6, dtype=torch.int64, device=self.device)

    def reset(self):
        self.acc.zero_()

    def update(self, output, labels, total_loss=None, two_stage=False):
        """one batch: output = the model's dict, labels = prep's label dict (mask_label, center_label, ...),
        total_loss = the criterion's 0-d float32 total on the device (or None)"""
        a, keep = _args(output, _label_fields(output, labels, two_stage), self.thr)
        _segmentation(a, output["logits"], labels["mask_label"], keep)
        if total_loss is not None:
            loss = total_loss.detach()
            if loss.dtype != torch.float32:
                loss = loss.float()
            keep.append(loss)
            a.loss = _hip.ptr(loss)
        a.acc = _hip.ptr(self.acc)
        _launch(a)

    def counts(self):
        """the raw accumulator (one device->host read): sums and integer counts"""
        w = self.acc.cpu()
        f = w[:3].view(torch.float64).tolist()
        n = w[3:].tolist()
        return {"sum_iou_bev": f[0], "sum_iou_3d": f[1], "sum_loss": f[2], "n_iou_3d_pass": n[0],
                "n_seg_correct": n[1], "n_samples": n[2]}

    def result(self):
        """(loss, seg_acc, iou2d, iou3d, iou3d_acc) as the reference divides them (by n_samples, and seg_acc by
        n_samples * n_points), plus the raw counts; one device->host read"""
        c = self.counts()
        n = c["n_samples"]
        div = (lambda x: x / n) if n else (lambda x: float("nan"))
        c.update(loss=div(c["sum_loss"]), seg_acc=(c["n_seg_correct"] / (n * float(self.n_points))) if n else float("nan"),
                 iou2d=div(c["sum_iou_bev"]), iou3d=div(c["sum_iou_3d"]), iou3d_acc=div(float(c["n_iou_3d_pass"])))
        return c
