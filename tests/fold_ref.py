"""The BatchNorm fold of the detector's MFMA layers (include/dal3.h, "The fold"; csrc/dal3_fold.h on the device),
restated once in numpy: rpn_ref.fold, sparse_ref.fold and roi_ref.fold forward here."""
import numpy as np


def fold(w, bias, bn, eps, channel_axis):
    """-> (W' float32 shaped like w, b' float32 (c_out)): float64 operations in include/dal3.h's order, each rounded by
    itself, one rounding to float32. channel_axis: the axis of w that is the output channel"""
    w64 = np.asarray(w, np.float64)
    b64 = np.zeros(w64.shape[channel_axis]) if bias is None else np.asarray(bias, np.float64)
    if bn is None:
        return w64.astype(np.float32), b64.astype(np.float32)
    g, beta, mean, var = (np.asarray(v, np.float64) for v in bn)
    scale = g / np.sqrt(var + eps)
    shape = [1] * w64.ndim
    shape[channel_axis] = -1
    return (w64 * scale.reshape(shape)).astype(np.float32), ((b64 - mean) * scale + beta).astype(np.float32)
