"""A MODEL of the dense stage on 16-bit MFMA operands (dal3_conv2d_lp of include/dal3.h; `precision` of rpn.RPN and
rpn.CenterHead), in the way tests/emu16.py models the point heads: what the arithmetic itself must cost, independently of
any kernel. Per layer, in this order: the BatchNorm fold bit for bit (rpn_ref.fold), the folded weight and the layer's
input rounded to the 16-bit type (round to nearest even, emu16.q's rounding), the layer in float64 from the rounded
operands with the float32 folded bias (rpn_ref.folded_layer), the result rounded to float32. `neck` and `head` chain
`layer` exactly as rpn_ref.neck_f64 and rpn_ref.head_f64 do, so every layer's input is rounded again. prec="fp32" rounds
nothing: the structure check. prec="f64" is the float64 truth itself (rpn_ref.layer from the unfolded parameters, nothing
rounded), and `cfg` / `order` are the neck's and the head's configuration (default: rpn_ref's production ones), so that a
detector with another neck (VoxelNet's) gets its truth and its model from its own state dict. `fault=` plants one wrong
rounding at a time (the CPU tests state what each must cost)."""
import numpy as np
import torch

import rpn_ref as R
from emu16 import DT

FAULTS = ("truncate", "weights_unrounded")
_BITS = {"fp16": 10, "bf16": 7}                 # stored mantissa bits


def q(x, prec):
    """round to the 16-bit type and back (RNE), as emu16.q does; numpy in, float32 numpy out"""
    x = np.ascontiguousarray(np.asarray(x, np.float32))
    if prec == "fp32":
        return x
    return torch.from_numpy(x.copy()).to(DT[prec]).float().numpy()          # (a copy: the shared fixtures are read-only)


def _truncated(x, prec):
    """the planted fault: the mantissa cut (toward zero) instead of rounded. Exact for the normal range of the type, which
    is where the fixtures live"""
    x = np.ascontiguousarray(np.asarray(x, np.float32))
    if prec == "fp32":
        return x
    return (x.view(np.uint32) & np.uint32(0xFFFFFFFF << (23 - _BITS[prec]) & 0xFFFFFFFF)).view(np.float32)


def layer(x, w, b, bn, eps, kind, stride, relu, prec, fault=None):
    if prec == "f64":
        return R.layer(x, w, b, bn, eps, kind, stride, relu)
    wf, bf = R.fold(w, b, bn, eps, deconv=kind == "deconv")
    rnd = _truncated if fault == "truncate" else q
    wq = wf if fault == "weights_unrounded" else rnd(wf, prec)
    return R.folded_layer(rnd(x, prec), wq, bf, kind, stride, relu).astype(np.float32)


def neck(sd, x, prec, fault=None, cfg=R.NECK):
    """rpn_ref.neck_f64's chain for the RPN configuration `cfg` -> (B, sum of us_num_filters, H, W) float32 (float64 for "f64")"""
    ups, start = [], len(cfg["layer_nums"]) - len(cfg["us_layer_strides"])
    for i, n in enumerate(cfg["layer_nums"]):
        for j in range(n + 1):
            x = layer(x, sd[f"blocks.{i}.{3 * j + 1}.weight"], None, R.bn_of(sd, f"blocks.{i}.{3 * j + 2}."), R.NECK_EPS, "3x3",
                      cfg["ds_layer_strides"][i] if j == 0 else 1, True, prec, fault)
        if i < start:
            continue
        s, k = cfg["us_layer_strides"][i - start], i - start
        ups.append(layer(x, sd[f"deblocks.{k}.0.weight"], None, R.bn_of(sd, f"deblocks.{k}.1."), R.NECK_EPS,
                         "1x1" if s == 1 else "deconv", s, True, prec, fault))
    return np.concatenate(ups, 1)


def head(sd, x, prec, fault=None, order=R.HEAD_ORDER, n_tasks=len(R.TASKS)):
    """rpn_ref.head_f64's chain (heads `order` per task) -> [ {head: (B, c, H, W) float32} per task ] (float64 for "f64")"""
    x = layer(x, sd["shared_conv.0.weight"], sd["shared_conv.0.bias"], R.bn_of(sd, "shared_conv.1."), R.HEAD_EPS, "3x3", 1, True,
              prec, fault)
    out = []
    for t in range(n_tasks):
        d = {}
        for name in order:
            p = f"tasks.{t}.{name}."
            y = layer(x, sd[p + "0.weight"], sd[p + "0.bias"], R.bn_of(sd, p + "1."), R.HEAD_EPS, "3x3", 1, True, prec, fault)
            d[name] = layer(y, sd[p + "3.weight"], sd[p + "3.bias"], None, R.HEAD_EPS, "3x3", 1, False, prec, fault)
        out.append(d)
    return out


def errors(got, truth):
    """-> {rms: rms(got - truth) / rms(truth), max: max |got - truth| / max |truth|} over the whole tensor"""
    truth = np.asarray(truth, np.float64)
    d = np.asarray(got).astype(np.float64) - truth
    return {"rms": float(np.sqrt((d ** 2).mean()) / np.sqrt((truth ** 2).mean())), "max": float(np.abs(d).max() / np.abs(truth).max())}
