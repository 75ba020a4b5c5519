"""A MODEL of the sparse 3-D middle on 16-bit MFMA operands (dal3_sp_conv_lp of include/dal3.h; `sparse_precision` of
sparse.SpMiddleResNetFHD), in the way tests/rpn_lp_model.py models the dense stage: what the arithmetic itself must cost,
independently of any kernel. Per layer, in this order: the BatchNorm fold bit for bit (sparse_ref.fold), the folded weight
and the layer's input rounded to the 16-bit type (rpn_lp_model.q: round to nearest even; the input as a float32 value
first, which is what the producing layer's float32 result is), the convolution from the rounded operands on
sparse_ref.Dense, the float32 folded bias, the residual UNROUNDED (the block input's own rows), ReLU, the mask. Everything
else is the backend's float64. `backbone` chains the layers exactly as sparse_ref.backbone does, so every layer's input
is rounded again. prec="f64" is the unrounded truth (sparse_ref's own layer from the unfolded parameters); prec="fp32"
rounds nothing: the structure check. `fault=` plants one wrong reading of the contract at a time; tests/test_sparse_lp_cpu.py
states what each must cost.

With a float32 backend (sparse_ref.Dense or sparse_ref.Rulebook) the same walk is the fp32 evaluation of the rounded
operands on the CPU: the single layers' yardstick. `layer_rows` is `layer` on the rulebook, row by row, for grids whose
dense map would be large."""
import numpy as np
import torch

import rpn_lp_model as M
import rpn_ref as R
import sparse_ref as S

FAULTS = ("truncate", "weights_unrounded", "residual_rounded", "inputs_unrounded")
q = M.q


def _rounder(prec, fault):
    return M._truncated if fault == "truncate" else M.q


def _round_map(be, x, prec, fault):
    """the backend's tensor with its values rounded to the 16-bit type (through float32), in the backend's dtype: a Dense's
    (map, mask) or a Rulebook's (rows, indices, shape)"""
    r = _rounder(prec, fault)
    if isinstance(be, S.Dense):
        return torch.from_numpy(np.ascontiguousarray(r(x[0].numpy(), prec))).to(be.dtype), x[1]
    return (np.asarray(r(x[0], prec), be.dtype),) + tuple(x[1:])


def step(be, x, w, bias, bn, kernel, stride, padding, subm, relu, prec, key, residual=None, fault=None, eps=S.EPS):
    """one layer on the backend's tensors (a Dense's (map, mask), a Rulebook's (rows, indices, shape)) -> the same kind.
    residual: the backend's map or rows, or None"""
    if prec == "f64":
        return S._post(be, be.conv(x, w, kernel, stride, padding, subm, key), bias, bn, eps, relu, residual)
    wf, bf = S.fold(w, bias, bn, eps)
    wq = wf if fault == "weights_unrounded" else _rounder(prec, fault)(wf, prec)
    xin = x if fault == "inputs_unrounded" else _round_map(be, x, prec, fault)
    if residual is not None and fault == "residual_rounded":
        residual = _round_map(be, (residual, None, None), prec, fault)[0]
    return S._post(be, be.conv(xin, wq, kernel, stride, padding, subm, key), bf, None, eps, relu, residual)


def layer(be, feats, idx, shape, w, bias, bn, kernel, stride, padding, subm, relu, prec, residual=False, fault=None, eps=S.EPS):
    """sparse_ref.layer's arguments plus `prec` -> the dense output (B, c_out, D', H', W') as a NumPy array. residual: add
    the input's own (unrounded) rows: a submanifold layer of equal widths"""
    x = be.start(feats, idx, shape)
    y = step(be, x, w, bias, bn, kernel, stride, padding, subm, relu, prec, "layer", be.feats(x) if residual else None, fault, eps)
    return np.asarray(be.dense(y))


def layer_rows(be, feats, idx, shape, w, bias, bn, kernel, stride, padding, subm, relu, prec, residual=False, fault=None, eps=S.EPS):
    """`layer` on a sparse_ref.Rulebook without the dense map -> (rows (n_out, c_out), output indices, output shape): a
    submanifold layer's rows in the input's order, a strided one's in key order"""
    x = be.start(feats, idx, shape)
    return step(be, x, w, bias, bn, kernel, stride, padding, subm, relu, prec, "layer", be.feats(x) if residual else None, fault, eps)


def backbone(sd, feats, idx, shape, prec, fault=None, B=None, be=None):
    """SpMiddleResNetFHD.forward on 16-bit operands from the unfolded parameters -> sparse_ref.backbone's dictionary
    ({"bev", "conv1" .. "conv4"}, float64). B: the batch size (default: the largest sample index + 1)"""
    if B is None:
        B = int(np.asarray(idx).reshape(-1, 4)[:, 0].max()) + 1
    be = S.Dense(B) if be is None else be
    x = be.start(feats, idx, shape)
    out, res = {}, 0
    for name, c, kernel, stride, padding in S.STEMS:
        subm = name == "conv_input"
        x = step(be, x, sd[f"{name}.0.weight"], None, R.bn_of(sd, f"{name}.1."), kernel, stride, padding, subm, True, prec,
                 "res0" if subm else name, None, fault)
        if name == "extra_conv":
            break
        seq, key = "conv1" if subm else name, f"res{res}"
        for j in ((0, 1) if subm else (3, 4)):
            p = f"{seq}.{j}."
            h = step(be, x, sd[p + "conv1.weight"], sd[p + "conv1.bias"], R.bn_of(sd, p + "bn1."), None, None, None, True, True,
                     prec, key, None, fault)
            x = step(be, h, sd[p + "conv2.weight"], sd[p + "conv2.bias"], R.bn_of(sd, p + "bn2."), None, None, None, True, True,
                     prec, key, be.feats(x), fault)
        out[seq] = np.asarray(be.dense(x))
        res += 1
    d = np.asarray(be.dense(x))
    Bn, C, D, H, W = d.shape
    out["bev"] = np.ascontiguousarray(d).reshape(Bn, C * D, H, W)
    return out


def inner_peak(sd, feats, idx, shape, B=None):
    """the largest magnitude any layer of the float64 chain takes as its input (the voxel features, every stem's and every
    block's outputs, and the blocks' inner activations): what fp16's range must hold"""
    if B is None:
        B = int(np.asarray(idx).reshape(-1, 4)[:, 0].max()) + 1
    be = _Peak(B)
    backbone(sd, feats, idx, shape, "f64", be=be)
    return be.peak


class _Peak(S.Dense):
    """sparse_ref.Dense that remembers the largest finite magnitude a convolution was given"""

    def __init__(self, B):
        super().__init__(B)
        self.peak = 0.0

    def conv(self, x, w, kernel, stride, padding, subm, key):
        v = torch.where(x[1], x[0], torch.zeros((), dtype=self.dtype)).abs()
        self.peak = max(self.peak, float(v[torch.isfinite(v)].max()) if v.numel() else 0.0)
        return super().conv(x, w, kernel, stride, padding, subm, key)


errors = M.errors
