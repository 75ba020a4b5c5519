"""The numpy side of tests/test_gpu_pack.py, without a GPU: the blob builders of tests/pack_ref.py invert (un-blob of
blob gives back the folded weights, and everything outside the layer is +0), and the three fold names of the stage
references return the bits of the one fold they forward to."""
import numpy as np
import pytest

import fold_ref
import pack_ref as K
import roi_ref
import rpn_ref
import sparse_ref


def _same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("case", range(len(K.DENSE)))
def test_dense_blob_inverts(case):
    kind, shape, axis, bias, bn = K.DENSE[case]
    w, b, stats, eps = K.layer_params(f"dense{case}", shape, axis, bias, bn)
    wf, bf = fold_ref.fold(w, b, stats, eps, axis)
    blob = K.dense_blob(wf, bf, kind)
    rows, c_in = (shape[0], shape[1]) if axis == 0 else (shape[1] * shape[2] * shape[3], shape[0])
    n_tiles, taps = -(-rows // 32), 9 if kind == "3x3" else 1
    assert blob.dtype == np.float32 and blob.size == n_tiles * 32 + n_tiles * -(-c_in // 8) * taps * 256
    w2, b2 = K.dense_unblob(blob, kind, shape)
    assert _same(w2, wf) and _same(b2, bf)
    assert np.count_nonzero(blob) == np.count_nonzero(wf) + K.SUB[kind] * np.count_nonzero(bf)


@pytest.mark.parametrize("case", range(len(K.SPARSE)))
def test_sparse_blob_inverts(case):
    shape, bias, bn = K.SPARSE[case]
    w, b, stats, eps = K.layer_params(f"sparse{case}", shape, -1, bias, bn)
    wf, bf = fold_ref.fold(w, b, stats, eps, -1)
    blob = K.sparse_blob(wf, bf)
    assert blob.dtype == np.float32 and not blob[:K.SP_HEAD].view(np.uint32).any()
    w2, b2 = K.sparse_unblob(blob, shape)
    assert _same(w2, wf) and _same(b2, bf)
    assert np.count_nonzero(blob) == np.count_nonzero(wf) + np.count_nonzero(bf)


@pytest.mark.parametrize("case", range(len(K.ROI)))
def test_roi_blob_is_the_layers_dense_blobs(case):
    layers = [fold_ref.fold(w[:, :, 0], b, stats, eps, 0) for w, b, stats, eps in K.roi_params(case)]
    blob, at = K.roi_blob(layers), 0
    for wf, bf in layers:
        n = -(-wf.shape[0] // 32) * (32 + -(-wf.shape[1] // 8) * 256)
        w2, b2 = K.dense_unblob(blob[at:at + n], "1x1", wf.shape + (1, 1))
        assert _same(w2[:, :, 0, 0], wf) and _same(b2, bf)
        at += n
    assert at == blob.size


def test_the_three_fold_names_agree_bit_for_bit():
    n = 0
    for case, (kind, shape, axis, bias, bn) in enumerate(K.DENSE):
        w, b, stats, eps = K.layer_params(f"dense{case}", shape, axis, bias, bn)
        want = fold_ref.fold(w, b, stats, eps, axis)
        got = rpn_ref.fold(w, b, stats, eps, deconv=axis == 1)
        assert _same(got[0], want[0]) and _same(got[1], want[1])
        if axis == 0:
            # the same layer as spconv holds it (taps..., c_in, c_out) and as a Conv1d over (c_in * taps)
            sp = sparse_ref.fold(np.ascontiguousarray(w.transpose(2, 3, 1, 0)), b, stats, eps)
            assert _same(np.ascontiguousarray(sp[0].transpose(3, 2, 0, 1)), want[0]) and _same(sp[1], want[1])
            ro = roi_ref.fold(w, b, stats, eps)
            assert _same(ro[0], want[0].reshape(shape[0], -1)) and _same(ro[1], want[1])
            n += 1
    for case, (shape, bias, bn) in enumerate(K.SPARSE):
        w, b, stats, eps = K.layer_params(f"sparse{case}", shape, -1, bias, bn)
        want = sparse_ref.fold(w, b, stats, eps)
        ro = roi_ref.fold(np.ascontiguousarray(np.moveaxis(w, -1, 0)), b, stats, eps)
        assert _same(ro[0], np.ascontiguousarray(np.moveaxis(want[0], -1, 0)).reshape(shape[-1], -1)) and _same(ro[1], want[1])
        n += 1
    for case in range(len(K.ROI)):
        for w, b, stats, eps in K.roi_params(case):
            want = roi_ref.fold(w, b, stats, eps)
            got = rpn_ref.fold(w[:, :, :, None], b, stats, eps)
            sp = sparse_ref.fold(np.ascontiguousarray(w[:, :, 0].T), b, stats, eps)
            assert _same(got[0][:, :, 0, 0], want[0]) and _same(got[1], want[1])
            assert _same(np.ascontiguousarray(sp[0].T), want[0]) and _same(sp[1], want[1])
            n += 1
    assert n == 3 + 3 + 6 + 5
