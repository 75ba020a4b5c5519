"""The sparse 3-D middle (3dal_pytorch_amd/sparse.py, dal3_sp_* of include/dal3.h) on the GPU: the bookkeeping against
sparse_ref's rulebook exactly, impulses bit for bit, single layers and the whole SpMiddleResNetFHD against the float64
truth with the torch-CPU fp32 masked dense evaluation as the yardstick (sparse_ref.BARS), NaN / Inf inputs, and the status
bits on inputs that are wrong by construction."""
import numpy as np
import pytest
import torch

import sparse_ref as S
from sparse_gpu import (GUARD, SENTINEL, Guarded, _dev, _hold, _record_file, backbone_module, backbone_truth, bn_module,  # noqa: F401
                        book_gpu, book_ref, conv_module, hip, run_layer, same_book, some_inactive, sparse, tensor)

pytestmark = pytest.mark.gpu
SMALL = (25, 7, 9)                              # the smallest depth every stem still fits: D 25 -> 13 -> 7 -> 3 -> 1


def _subset(tag, n, B, shape):
    """n distinct sites of B x shape in a seeded scrambled order"""
    cells = B * int(np.prod(shape))
    order = np.argsort(S.synth.uniform(S.SEED, f"subset/{tag}", (cells,)), kind="stable")[:n]
    return S.unkey(order, shape)


def _corners(shape):
    D, H, W = shape
    return [[0, z, y, x] for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]


BOOK_CASES = {
    "corners": (np.asarray(_corners(SMALL), np.int32), 1, SMALL),
    "full_3x4x5": (S.unkey(np.arange(60)[::-1].copy(), (3, 4, 5)), 1, (3, 4, 5)),
    "b3_sample1_empty": (np.concatenate([_subset("b3/0", 90, 1, SMALL), _subset("b3/2", 70, 1, SMALL) + np.asarray([2, 0, 0, 0], np.int32)]), 3, SMALL),
    **{f"n{n}": (_subset(f"n{n}", n, 2, SMALL), 2, SMALL) for n in (1, 31, 32, 33, 63, 64, 65, 300)},
}


@pytest.mark.parametrize("name", sorted(BOOK_CASES))
def test_bookkeeping_is_the_rulebooks(name):
    idx, B, shape = BOOK_CASES[name]
    n = idx.shape[0]
    want = book_ref(idx, B, shape)
    ref = None
    for mw in (0, 1, 3):
        # capacity beyond the count: rows behind it are sentinels the kernels must leave alone
        x = tensor(np.zeros((n, 1), np.float32), idx, B, shape, capacity=n + 37, n=n)
        got, intact = book_gpu(x, max_workgroups=mw)
        assert intact and int(x.status.item()) == 0
        same_book(got, want)
        # (level 0's rows behind n are the caller's, and its table's columns there are never written)
        flat = [got[0][4][:, :n]] + [a for g in got[1:] for a in (g[1], g[4], g[5])]
        if ref is None:
            ref = flat
        else:
            assert all(np.array_equal(a, b) for a, b in zip(flat, ref)), f"max_workgroups {mw} changes the bytes"


def test_overflow_sets_the_bit_and_stays_in_bounds():
    idx, B, shape = BOOK_CASES["n300"]
    want = book_ref(idx, B, shape)
    full = want[1][1].shape[0]
    cap = full - 50
    x = tensor(np.zeros((300, 1), np.float32), idx, B, shape)
    got, intact = book_gpu(x, caps={"conv2": cap})
    assert intact
    assert int(x.status.item()) == hip.SP_OVERFLOW
    name, gi, gn, _, _, _, c = got[1]
    assert (name, gn, c) == ("conv2", cap, cap) and np.array_equal(gi, want[1][1][:cap])      # the first sites by key survive
    for _, gi, gn, gshape, g27, gdown, c in got[2:]:                                          # later levels: in bounds
        assert 0 <= gn <= c and (g27[:, :gn] < gn).all() and (gi[:gn] >= 0).all() and (gi[:gn, 1:] < np.asarray(gshape)).all()


def test_bad_coordinate_and_duplicate_set_their_bits():
    idx, B, shape = BOOK_CASES["n65"]
    bad = idx.copy()
    bad[10, 3], bad[50, 0] = shape[2], B                    # one past the grid, one past the batch
    w, b, bn = S.layer_weights("badcoord", (3, 3, 3), 5, 16, False, True)
    feats = S.synth.uniform(S.SEED, "badcoord/x", (65, 5), 0.0, 2.0).astype(np.float32)
    x = tensor(feats, bad, B, shape)
    got, y = run_layer(x, w, b, bn, (3, 3, 3), (1, 1, 1), (1, 1, 1), True, True)
    assert int(x.status.item()) == hip.SP_BAD_COORD
    rows = y.features.cpu().numpy()
    assert not rows[[10, 50]].any() and not np.signbit(rows[[10, 50]]).any()       # +0
    keep = np.ones(65, bool)
    keep[[10, 50]] = False
    truth = S.layer(S.Dense(B), feats[keep], bad[keep], shape, w, b, bn, (3, 3, 3), (1, 1, 1), (1, 1, 1), True, True)
    f32 = S.layer(S.Dense(B, torch.float32), feats[keep], bad[keep], shape, w, b, bn, (3, 3, 3), (1, 1, 1), (1, 1, 1), True, True)
    _hold("bad_coord/absent", got, f32, truth)
    # the strided levels do not see the bad rows either
    levels, intact = book_gpu(tensor(feats, bad, B, shape))
    same_book(levels[1:], book_ref(bad, B, shape)[1:])      # (the rulebook treats a row outside the grid as absent)
    assert intact

    dup = idx.copy()
    dup[20] = dup[3]
    x = tensor(feats, dup, B, shape)
    levels, intact = book_gpu(x)
    assert intact and int(x.status.item()) == hip.SP_DUPLICATE
    for _, gi, gn, gshape, g27, gdown, c in levels[1:]:
        assert 0 <= gn <= c and (g27[:, :gn] < gn).all()


def test_a_non_finite_folded_weight_is_refused():
    idx, B, shape = BOOK_CASES["n33"]
    w, b, bn = S.layer_weights("badw", (3, 3, 3), 16, 16, True, True)
    w = w.copy()
    w[1, 1, 1, 3, 5] = np.inf
    conv = conv_module(w, b, (3, 3, 3), (1, 1, 1), (1, 1, 1), True)
    status = torch.zeros(1, dtype=torch.int32).cuda()
    packed = sparse.pack_layer(conv, bn_module(bn), status)
    assert int(status.item()) == hip.SP_BAD_WEIGHT
    x = tensor(np.ones((33, 16), np.float32), idx, B, shape)
    out = torch.full((33, 16), float(SENTINEL)).cuda()
    sparse.conv(x.features, sparse.subm_table(x), x.n, packed, 16, 16, x.status, out=out)
    assert int(x.status.item()) == hip.SP_BAD_WEIGHT and bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------- impulses, bit for bit
FORMS = {"subm": ((3, 3, 3), (1, 1, 1), (1, 1, 1), True), "k3s2p1": ((3, 3, 3), (2, 2, 2), (1, 1, 1), False),
         "k3s2p011": ((3, 3, 3), (2, 2, 2), (0, 1, 1), False), "k311s211": ((3, 1, 1), (2, 1, 1), (0, 0, 0), False)}
IMPULSE_GRID = (5, 7, 9)                        # odd extents: the stride-2 phase and the floor in the extent show


@pytest.mark.parametrize("form", ("subm", "k3s2p1", "k3s2p011", "k311s211", "canvas"))
def test_impulses_bit_for_bit(form):
    canvas = form == "canvas"                   # the last layer's store, on the last layer's form
    kernel, stride, padding, subm = FORMS["k311s211" if canvas else form]
    B, shape = 1, IMPULSE_GRID
    D, H, W = shape
    idx = S.unkey(np.arange(D * H * W), shape)              # fully active, rows in key order: row = key
    n = idx.shape[0]
    w, b, bn = S.layer_weights(f"impulse/{form}", kernel, 6, 32, True, True)
    wf, bf = S.fold(w, b, bn)
    osh = S.out_shape(shape, kernel, stride, padding)
    oidx = idx if subm else S.downsample(idx, B, shape, kernel, stride, padding)[0]
    t = S.table(oidx, idx, B, shape, osh, kernel, stride, padding)
    assert oidx.shape[0] > 32
    # corners, a face, the interior, and the input rows under output rows 31 and 32: either side of a tile seam
    seam = [int(t[t.shape[0] // 2, 31]), int(t[t.shape[0] // 2, 32])]
    at = [0, n - 1, W - 1, (H - 1) * W, (D // 2) * H * W, ((D // 2) * H + H // 2) * W + W // 2] + [s for s in seam if s >= 0]
    for j, p in enumerate(at):
        c = j % 6
        feats = np.zeros((n, 6), np.float32)
        feats[p, c] = 1.0
        want = np.repeat(np.maximum(bf, 0)[None, :], oidx.shape[0], 0)
        for tap, o in zip(*np.nonzero(t == p)):
            want[o] = np.maximum(wf.reshape(-1, 6, 32)[tap, c] + bf, np.float32(0))
        dense = np.zeros((B, *osh, 32), np.float32)
        dense[oidx[:, 0], oidx[:, 1], oidx[:, 2], oidx[:, 3]] = want
        got, _ = run_layer(tensor(feats, idx, B, shape), w, b, bn, kernel, stride, padding, subm, True, canvas=canvas)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), dense.transpose(0, 4, 1, 2, 3).view(np.uint32)), (form, p)


# ------------------------------------------------------------------------------------- single layers against float64
PAIRS = ((5, 16), (6, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128))
LAYER_GRID = (11, 13, 15)
LAYER_FORMS = ("subm", "k3s2p1", "k3s2p011", "k311s211", "canvas")


@pytest.mark.parametrize("form", LAYER_FORMS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_single_layers_against_float64(pair, form):
    c_in, c_out = pair
    kernel, stride, padding, subm = FORMS["k311s211" if form == "canvas" else form]
    v = PAIRS.index(pair) + LAYER_FORMS.index(form)          # the variants walk through bias / BatchNorm / ReLU / residual
    bias, use_bn, relu = bool(v & 1), bool(v & 2) or not (v & 1), not (v % 3 == 0)
    residual = subm and c_in == c_out and bool(v & 1)
    B, shape = 2, LAYER_GRID
    idx = S.batch([S.clustered(f"layer/{c_in}/0", shape, 2, 90, 1.6), S.clustered(f"layer/{c_in}/1", shape, 1, 60, 1.2)])
    feats = S.synth.uniform(S.SEED, f"layer/{c_in}/x", (idx.shape[0], c_in), 0.0, 2.0).astype(np.float32)
    w, b, bn = S.layer_weights(f"layer/{c_in}-{c_out}/{form}", kernel, c_in, c_out, bias, use_bn)
    args = (feats, idx, shape, w, b, bn, kernel, stride, padding, subm, relu, residual)
    truth = S.layer(S.Dense(B), *args)
    f32 = S.layer(S.Dense(B, torch.float32), *args)
    some_inactive(S.layer(S.Dense(B), feats, idx, shape, np.ones_like(w), None, None, kernel, stride, padding, subm, False), form)
    got, _ = run_layer(tensor(feats, idx, B, shape), w, b, bn, kernel, stride, padding, subm, relu, residual, canvas=form == "canvas")
    assert got.shape == truth.shape
    inactive = np.abs(S.layer(S.Dense(B), feats, idx, shape, np.ones_like(w), None, None, kernel, stride, padding, subm, False)).max(1) == 0
    cells = np.moveaxis(got, 1, -1)[inactive]
    assert not cells.any() and not np.signbit(cells).any()                 # inactive cells are +0 exactly
    _hold(f"layer/{c_in}-{c_out}/{form}", got, f32, truth)


# ------------------------------------------------------------------------------------- the whole backbone
def _run_backbone(c_in, feats, idx, B, shape, **kw):
    m = backbone_module(c_in)
    voxel_shape = [shape[2], shape[1], shape[0] - 1]        # input_shape is the voxel grid [x, y, z]; the module adds 1 to z
    with torch.no_grad():
        bev, levels = m(_dev(feats), _dev(idx), B, voxel_shape, **kw)
    return m, bev, levels


@pytest.mark.parametrize("c_in", (5, 6))
def test_backbone_against_float64(c_in):
    feats, idx, B, shape, truth, f32 = backbone_truth(c_in)
    for k in ("bev",) + S.LEVELS:
        some_inactive(truth[k][:1], k)
    m, bev, levels = _run_backbone(c_in, feats, idx, B, shape)
    assert int(m.last_status.item()) == 0
    got = bev.cpu().numpy()
    assert got.shape == (3, 256, 5, 6)
    inactive = np.abs(truth["bev"]).max(1) == 0
    cells = np.moveaxis(got, 1, -1)[inactive]
    assert not cells.any() and not np.signbit(cells).any()
    _hold(f"backbone/{c_in}/bev", got, f32["bev"], truth["bev"])
    assert list(levels) == list(S.LEVELS)
    for k in S.LEVELS:
        _hold(f"backbone/{c_in}/{k}", levels[k].dense().cpu().numpy(), f32[k], truth[k])
    # the bits depend on neither the grid nor the capacity
    for mw in (1, 3):
        _, bev2, levels2 = _run_backbone(c_in, feats, idx, B, shape, max_workgroups=mw)
        assert torch.equal(bev, bev2) and all(torch.equal(levels[k].dense(), levels2[k].dense()) for k in S.LEVELS)


def test_backbone_is_refused_in_train_mode_and_enqueues_without_a_synchronisation():
    feats, idx, B, shape, _, _ = backbone_truth(5)
    m = backbone_module(5)
    df, di = _dev(feats), _dev(idx)
    n = torch.tensor([idx.shape[0]], dtype=torch.int64).cuda()
    m.packed()
    for s in ("conv1", "conv2", "conv3", "conv4"):
        for blk in getattr(m, s):
            if isinstance(blk, sparse.SparseBasicBlock):
                blk.packed()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            bev, _ = m(df, di, B, [shape[2], shape[1], shape[0] - 1], n_voxels=n)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    with torch.no_grad():
        assert torch.equal(bev, m(df, di, B, [shape[2], shape[1], shape[0] - 1])[0])
    with pytest.raises(RuntimeError, match="eval-mode"):
        m.train()(df, di, B, [shape[2], shape[1], shape[0] - 1])


def test_nan_and_inf_reach_what_the_truth_says():
    feats, idx, B, shape, truth, f32 = backbone_truth(5, True)
    assert not np.isfinite(truth["bev"]).all() and np.isfinite(truth["bev"]).any()
    assert not np.isfinite(truth["bev"][2]).all() and np.isfinite(truth["bev"][0]).all()       # the clustered sample is the finite rest
    m, bev, levels = _run_backbone(5, feats, idx, B, shape)
    for k, got in [("bev", bev.cpu().numpy())] + [(k, levels[k].dense().cpu().numpy()) for k in S.LEVELS]:
        g, t = S.finite_part(got, truth[k])
        y, _ = S.finite_part(f32[k], truth[k])
        _hold(f"nonfinite/{k}", g, y, t)
