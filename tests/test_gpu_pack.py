"""The packed-weight blobs of the detector's MFMA layers on the GPU, word for word: what rpn.pack_layer (dal3_conv2d_pack),
sparse.pack_layer (dal3_sp_conv_pack) and RoIHead.packed() (dal3_roi_pack) write against the numpy blobs that
tests/pack_ref.py builds from the one reference fold (tests/fold_ref.py) and the layouts the kernels' header comments
document. The cases (pack_ref.DENSE / SPARSE / ROI) are the smallest shapes that reach every branch of the packers."""
import importlib

import numpy as np
import pytest
import torch
from torch import nn

import fold_ref
import pack_ref as K

pytestmark = pytest.mark.gpu

hip = importlib.import_module("3dal_pytorch_amd._hip")
rpn = importlib.import_module("3dal_pytorch_amd.rpn")
sparse = importlib.import_module("3dal_pytorch_amd.sparse")
two_stage = importlib.import_module("3dal_pytorch_amd.two_stage")
KINDS = {"3x3": hip.CONV2D_3X3, "1x1": hip.CONV2D_1X1, "deconv2": hip.CONV2D_DECONV2, "deconv4": hip.CONV2D_DECONV4}


def _set(t, v):
    t.data = torch.from_numpy(np.ascontiguousarray(v))


def _norm(cls, stats, eps):
    if stats is None:
        return None
    m = cls(len(stats[0]), eps=eps)
    for t, v in zip((m.weight, m.bias, m.running_mean, m.running_var), stats):
        _set(t, v)
    return m.cuda().eval()


def _words_equal(got, want):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{bad.size} of {want.size} words differ, the first at {bad[0]}: {got[bad[0]]!r} for {want[bad[0]]!r}"


@pytest.mark.parametrize("case", range(len(K.DENSE)))
def test_dense_blob_word_for_word(case):
    kind, shape, axis, bias, bn = K.DENSE[case]
    w, b, stats, eps = K.layer_params(f"dense{case}", shape, axis, bias, bn)
    if axis == 1:
        conv = nn.ConvTranspose2d(shape[0], shape[1], shape[2], stride=shape[2], bias=bias)
    else:
        conv = nn.Conv2d(shape[1], shape[0], shape[2], padding=shape[2] // 2, bias=bias)
    _set(conv.weight, w)
    if bias:
        _set(conv.bias, b)
    got = rpn.pack_layer(conv.cuda().eval(), _norm(nn.BatchNorm2d, stats, eps), KINDS[kind])
    _words_equal(got, K.dense_blob(*fold_ref.fold(w, b, stats, eps, axis), kind))


@pytest.mark.parametrize("case", range(len(K.SPARSE)))
def test_sparse_blob_word_for_word(case):
    shape, bias, bn = K.SPARSE[case]
    w, b, stats, eps = K.layer_params(f"sparse{case}", shape, -1, bias, bn)
    conv = sparse.SubMConv3d(shape[3], shape[4], shape[:3], bias=bias) if shape[:3] == (3, 3, 3) else \
        sparse.SparseConv3d(shape[3], shape[4], shape[:3], stride=(2, 1, 1), bias=bias)
    _set(conv.weight, w)
    if bias:
        _set(conv.bias, b)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = sparse.pack_layer(conv.cuda().eval(), _norm(nn.BatchNorm1d, stats, eps), status)
    assert not got[:K.SP_HEAD].cpu().numpy().view(np.uint32).any(), "the 64-float head (word 0: the non-finite flag) is not +0"
    assert int(status.item()) == 0
    _words_equal(got, K.sparse_blob(*fold_ref.fold(w, b, stats, eps, -1)))


@pytest.mark.parametrize("case", range(len(K.ROI)))
def test_roi_blob_is_the_layers_dense_blobs(case):
    c_in, shared, cls, reg, code = K.ROI[case]
    head = two_stage.RoIHead(c_in, dict(SHARED_FC=list(shared), CLS_FC=list(cls), REG_FC=list(reg), DP_RATIO=0.3), code_size=code)
    params = K.roi_params(case)
    convs = [m for seq in (head.shared_fc_layer, head.cls_layers, head.reg_layers) for m in seq if isinstance(m, nn.Conv1d)]
    norms = [m for seq in (head.shared_fc_layer, head.cls_layers, head.reg_layers) for m in seq if isinstance(m, nn.BatchNorm1d)]
    assert len(convs) == len(params) and len(norms) == sum(p[2] is not None for p in params)
    norms = iter(norms)
    for conv, (w, b, stats, eps) in zip(convs, params):
        assert tuple(conv.weight.shape) == w.shape and (conv.bias is None) == (b is None)
        _set(conv.weight, w)
        if b is not None:
            _set(conv.bias, b)
        if stats is not None:
            m = next(norms)
            m.eps = eps
            for t, v in zip((m.weight, m.bias, m.running_mean, m.running_var), stats):
                _set(t, v)
    head = head.cuda().eval()
    layers = [fold_ref.fold(w[:, :, 0], b, stats, eps, 0) for w, b, stats, eps in params]
    want = np.concatenate([K.dense_blob(wf[:, :, None, None], bf, "1x1") for wf, bf in layers])
    assert np.array_equal(want.view(np.uint32), K.roi_blob(layers).view(np.uint32))
    _words_equal(head.packed(), want)
