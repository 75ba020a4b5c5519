"""What tests/test_gpu_rpn.py and tests/test_gpu_detector.py share: single layers through dal3_conv2d, the production
modules with the seeded weights, references computed once, and the record of every figure held under
DAL3_RPN_RECORD=<path> (how profiles/rpn_measured.json is made: run both files in one session)."""
import functools
import importlib
import json
import os

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import rpn_ref as R

hip = importlib.import_module("3dal_pytorch_amd._hip")
rpn = importlib.import_module("3dal_pytorch_amd.rpn")
_RECORD = {}
KINDS = {("3x3", 1): hip.CONV2D_3X3, ("3x3", 2): hip.CONV2D_3X3, ("1x1", 1): hip.CONV2D_1X1, ("deconv", 2): hip.CONV2D_DECONV2,
         ("deconv", 4): hip.CONV2D_DECONV4}


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """imported by both test files: each writes all the figures held so far when its last test is done"""
    yield
    path = os.environ.get("DAL3_RPN_RECORD")
    if path and _RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _hold(row, got, f32, truth):
    """pillars_gpu._hold's rule: each measure <= bar x the fp32 yardstick's own error against the truth, dead channels +0"""
    ratio, m, y = R.ratios(got, f32, truth)
    _RECORD[row] = {"measured": {k: m[k] for k in R.MEASURES}, "yardstick": {k: y[k] for k in R.MEASURES}, "ratio": ratio}
    for k in R.MEASURES:
        print(f"{row:34s} {k:9s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:7.2f}  bar {R.BARS[k]:g}")
    assert m["dead_ok"]
    bad = [(k, m[k], ratio[k]) for k in R.MEASURES if ratio[k] > R.BARS[k]]
    assert not bad, (row, bad)


def layer_params(tag, kind, stride, c_in, c_out, bias, bn):
    """seeded parameters of one layer -> (w, bias or None, (g, beta, mean, var) or None)"""
    taps = 9 if kind == "3x3" else 1
    shape = (c_in, c_out, stride, stride) if kind == "deconv" else (c_out, c_in, 3, 3) if kind == "3x3" else (c_out, c_in, 1, 1)
    w = R._w(tag, shape, c_in * taps, deconv=kind == "deconv")
    b = R.synth.uniform(R.SEED, tag + "/bias", (c_out,), -0.5, 0.5).astype(np.float32) if bias else None
    sd = {}
    if bn:
        R._bn(sd, "", tag, c_out)
    return w, b, (R.bn_of(sd, "") if bn else None)


def torch_layer(w, b, bn, eps, kind, stride, device="cpu"):
    """the layer as the reference builds it: nn.Conv2d / nn.ConvTranspose2d (+ nn.BatchNorm2d), eval mode"""
    if kind == "deconv":
        conv = nn.ConvTranspose2d(w.shape[0], w.shape[1], stride, stride=stride, bias=b is not None)
    else:
        conv = nn.Conv2d(w.shape[1], w.shape[0], w.shape[2], stride=stride, padding=w.shape[2] // 2, bias=b is not None)
    conv.weight.data = torch.from_numpy(w)
    if b is not None:
        conv.bias.data = torch.from_numpy(b)
    norm = None
    if bn is not None:
        norm = nn.BatchNorm2d(conv.out_channels, eps=eps)
        for t, v in zip((norm.weight, norm.bias, norm.running_mean, norm.running_var), bn):
            t.data = torch.from_numpy(np.asarray(v))
    return conv.to(device).eval(), (norm.to(device).eval() if norm is not None else None)


@torch.no_grad()
def yardstick(x, w, b, bn, eps, kind, stride, relu):
    """the torch-CPU fp32 layer"""
    conv, norm = torch_layer(w, b, bn, eps, kind, stride)
    y = conv(torch.from_numpy(np.ascontiguousarray(x)))
    if norm is not None:
        y = norm(y)
    return (F.relu(y) if relu else y).numpy()


@torch.no_grad()
def run_layer(x_dev, w, b, bn, eps, kind, stride, relu, **kw):
    """fold + pack + one dal3_conv2d launch -> the output view (device)"""
    conv, norm = torch_layer(w, b, bn, eps, kind, stride, "cuda")
    packed = rpn.pack_layer(conv, norm, KINDS[kind, stride])
    return rpn.conv2d(x_dev, packed, KINDS[kind, stride], stride, relu, conv.out_channels, **kw)


def load(mod, sd, device="cuda"):
    mod.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return mod.to(device).eval()


def neck_module(device="cuda"):
    return load(rpn.RPN(**R.NECK), R.neck_weights(), device)


def head_module(device="cuda"):
    return load(rpn.CenterHead(**R.HEAD), R.head_weights(), device)


BIG = (2, 64, 36, 44)


@functools.lru_cache(maxsize=None)
def dense_case(tag):
    """canvas `tag` ('a', 'b' of the fixture, or 'big') -> (x, neck truth, neck fp32, head truth, head fp32): the float64
    restatement and the torch-CPU composite, computed once and shared (read-only)"""
    x = R.canvas(tag, BIG if tag == "big" else R.CANVASES[tag])
    n64 = R.neck_f64(R.neck_weights(), x)
    h64 = R.head_cat(R.head_f64(R.head_weights(), n64))
    with torch.no_grad():
        n32 = neck_module("cpu").composite(torch.from_numpy(x))
        h32 = head_module("cpu").composite(n32)
    out = (x, n64, n32.numpy(), h64, R.head_cat([{k: v.numpy() for k, v in d.items()} for d in h32]))
    for a in out:
        a.setflags(write=False)
    return out
