"""The sparse backbone's training pass on the GPU (sparse.py's train_forward; dal3_sp_table_transposed and dal3_sp_wgrad of
include/dal3.h): the transposed table against the rulebook's inverse exactly, weight-gradient impulses bit for bit, the
gradients of single layers, of a block, of the whole SpMiddleResNetFHD and of VoxelNet.first_stage_loss against the float64
truth with the torch-CPU fp32 masked dense autograd as the yardstick (sparse_train_ref.BARS), dead rows, the K-slice seam
and the bits under every grid. Every figure held is recorded under DAL3_SPARSE_TRAIN_RECORD=<path>
(how profiles/sparse_train_measured.json is made)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import sparse_ref as S
import sparse_train_ref as T
from sparse_gpu import GUARD, SENTINEL, Guarded, _dev, backbone_module, conv_module, hip, some_inactive, sparse, tensor  # noqa: F401

pytestmark = pytest.mark.gpu
SMALL = (25, 7, 9)
FORMS = {"subm": ((3, 3, 3), (1, 1, 1), (1, 1, 1), True), "k3s2p1": ((3, 3, 3), (2, 2, 2), (1, 1, 1), False),
         "k3s2p011": ((3, 3, 3), (2, 2, 2), (0, 1, 1), False), "k311s211": ((3, 1, 1), (2, 1, 1), (0, 0, 0), False)}
_RECORD = {}


@pytest.fixture(autouse=True)
def _grad_on():
    """whatever a test before this file left switched"""
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    path = os.environ.get("DAL3_SPARSE_TRAIN_RECORD")
    if path and _RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


def _hold(row, got, f32, truth, bars=None):
    """each measure <= bar x the fp32 yardstick's own error against the truth, dead channels +0"""
    bars = T.BARS if bars is None else bars
    ratio, m, y = S.P.ratios(T.as_rows(got), T.as_rows(f32), T.as_rows(truth))
    _RECORD[row] = {"measured": {k: m[k] for k in T.MEASURES}, "yardstick": {k: y[k] for k in T.MEASURES}, "ratio": ratio}
    for k in T.MEASURES:
        print(f"{row:44s} {k:9s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:7.2f}  bar {bars[k]:g}")
    assert m["dead_ok"], row
    bad = [(k, m[k], ratio[k]) for k in T.MEASURES if ratio[k] > bars[k]]
    assert not bad, (row, bad)


def _subset(tag, n, B, shape):
    """n distinct sites of B x shape in a seeded scrambled order"""
    cells = B * int(np.prod(shape))
    order = np.argsort(S.synth.uniform(S.SEED, f"trsubset/{tag}", (cells,)), kind="stable")[:n]
    return S.unkey(order, shape)


def _plus_zero(a):
    a = np.asarray(a)
    return not a.any() and not np.signbit(a).any()


# ------------------------------------------------------------------------------------- the transposed table
def _walk_transposed(x, caps=None, mw=0):
    """every strided level's transposed table on the device, in guarded sentinel-filled buffers -> ([(name, table
    (taps, in_capacity), n_in, out indices, n_out)], guards intact)"""
    caps, out, bufs = caps or {}, [], []
    from sparse_gpu import windows
    for name, kernel, stride, padding, osh in windows(x.spatial_shape):
        cap = caps.get(name, sparse.safe_capacity(x.capacity, x.batch_size, x.spatial_shape, kernel, stride, padding))
        gi, gk = Guarded(cap, 4), Guarded(cap, 0)
        indices, keys, n_out, cap, shape = sparse.downsample(x, kernel, stride, padding, cap, mw, gi.view, gk.view)
        taps = int(np.prod(kernel))
        gt = Guarded(taps * x.capacity, 0)
        inv = sparse.transposed_table(x, keys, n_out, cap, shape, kernel, stride, padding, mw, gt.view.view(taps, x.capacity))
        bufs += [gi, gk, gt]
        n_in = x.capacity if x.n is None else int(x.n.item())
        out.append((name, inv.cpu().numpy(), n_in, indices.cpu().numpy(), int(n_out.item())))
        y = sparse.SparseConvTensor(torch.zeros((cap, 1), dtype=torch.float32).cuda(), indices, shape, x.batch_size, n_out, x.status)
        y.sorted = (keys, None)
        x = y
    return out, all(b.intact() for b in bufs)


def _inverse_ref(idx, B, shape, keep=None):
    """the rulebook's inverse of every strided level; keep: {name: the first sites by key that an overflowed level keeps}"""
    from sparse_gpu import windows
    out = []
    for name, kernel, stride, padding, osh in windows(shape):
        o, _ = S.downsample(idx, B, shape, kernel, stride, padding)
        o = o[:(keep or {}).get(name, o.shape[0])]
        out.append((name, T.inverse_table(idx, o, B, shape, osh, kernel, stride, padding), o))
        idx, shape = o, osh
    return out


@pytest.mark.parametrize("n", (1, 31, 32, 33, 63, 64, 65, 300))
def test_transposed_table_is_the_rulebooks_inverse(n):
    B, shape = 2, SMALL
    idx = _subset(f"n{n}", n, B, shape)
    want = _inverse_ref(idx, B, shape)
    assert len(want) == 4
    ref = None
    for mw in (0, 1, 3):
        x = tensor(np.zeros((n, 1), np.float32), idx, B, shape, capacity=n + 37, n=n)
        got, intact = _walk_transposed(x, mw=mw)
        assert intact and int(x.status.item()) == 0
        for (name, inv, n_in, oidx, n_out), (wname, winv, wo) in zip(got, want):
            assert name == wname and n_in == winv.shape[1] and n_out == wo.shape[0], name
            assert np.array_equal(inv[:, :n_in], winv), (name, mw)
            assert (inv[:, n_in:] == SENTINEL).all(), name          # columns behind the count are never written
        flat = [g[1][:, :g[2]] for g in got]
        if ref is None:
            ref = flat
        else:
            assert all(np.array_equal(a, b) for a, b in zip(flat, ref)), f"max_workgroups {mw} changes the bytes"


def test_transposed_table_of_an_overflowed_level_stays_in_bounds():
    B, shape = 2, SMALL
    idx = _subset("n300", 300, B, shape)
    full = S.downsample(idx, B, shape, (3, 3, 3), (2, 2, 2), (1, 1, 1))[0].shape[0]
    cap = full - 50
    x = tensor(np.zeros((300, 1), np.float32), idx, B, shape)
    got, intact = _walk_transposed(x, caps={"conv2": cap})
    assert intact and int(x.status.item()) == hip.SP_OVERFLOW
    want = _inverse_ref(idx, B, shape, keep={"conv2": cap})
    for (name, inv, n_in, oidx, n_out), (_, winv, wo) in zip(got, want):
        assert n_out == wo.shape[0] and np.array_equal(inv[:, :n_in], winv), name      # a dropped site is simply absent
        assert (inv[:, :n_in] >= -1).all() and (inv[:, :n_in] < n_out).all(), name
    assert got[0][4] == cap and (got[0][1][:, :300] < 0).all(0).any()          # some input sites lost every output site


# ------------------------------------------------------------------------------------- wgrad impulses, bit for bit
def _tables(x, kernel, stride, padding, subm, mw=0):
    """-> (forward table, n_out, out capacity) of one layer on the device"""
    if subm:
        return sparse.subm_table(x, None, mw), x.n, x.capacity
    indices, keys, n_out, cap, shape = sparse.downsample(x, kernel, stride, padding, None, mw)
    return sparse.neighbour_table(x, indices, n_out, cap, shape, kernel, stride, padding, mw), n_out, cap


@pytest.mark.parametrize("form", sorted(FORMS))
def test_wgrad_impulses_bit_for_bit(form):
    kernel, stride, padding, subm = FORMS[form]
    B, shape = 1, (5, 7, 9)
    D, H, W = shape
    idx = S.unkey(np.arange(D * H * W), shape)              # fully active, rows in key order: row = key
    n = idx.shape[0]
    osh = S.out_shape(shape, kernel, stride, padding)
    oidx = idx if subm else S.downsample(idx, B, shape, kernel, stride, padding)[0]
    t = S.table(oidx, idx, B, shape, osh, kernel, stride, padding)
    taps, n_out = t.shape
    assert n_out > 32
    seam = [int(t[taps // 2, 31]), int(t[taps // 2, 32])]
    at = [0, n - 1, W - 1, (H - 1) * W, (D // 2) * H * W, ((D // 2) * H + H // 2) * W + W // 2] + [s for s in seam if s >= 0]
    for c_in, c_out in ((6, 32), (64, 16)):
        dy = S.synth.normal(S.SEED, f"wimpulse/{form}/{c_out}", (n_out, c_out), 0.0, 1.0).astype(np.float32)
        x = tensor(np.zeros((n, c_in), np.float32), idx, B, shape)
        table, n_dev, cap = _tables(x, kernel, stride, padding, subm)
        assert cap >= n_out and np.array_equal(table.cpu().numpy()[:, :n_out], t)
        ddy = torch.zeros((cap, c_out), dtype=torch.float32).cuda()
        ddy[:n_out] = _dev(dy)
        for j, p in enumerate(at):
            c = (7 * j + 3) % c_in
            feats = torch.zeros((n, c_in), dtype=torch.float32).cuda()
            feats[p, c] = 1.0
            dw, db = sparse.wgrad(feats, table, n_dev, ddy, kernel)
            want = np.zeros((taps, c_in, c_out), np.float32)
            for tap, o in zip(*np.nonzero(t == p)):
                want[tap, c] = dy[o]                        # the one output site that reads p under this tap
            assert (np.count_nonzero(t == p, 1) <= 1).all() and (t == p).any()
            got = dw.cpu().numpy().reshape(taps, c_in, c_out)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (form, c_in, p)
            assert db.shape == (c_out,) and np.allclose(db.cpu().numpy(), dy.astype(np.float64).sum(0), rtol=0, atol=1e-4)


# ------------------------------------------------------------------------------------- single layers against float64
PAIRS = ((5, 16), (16, 16), (16, 32), (32, 64), (64, 128), (128, 128))
LAYER_GRID = (11, 13, 15)


def _layer_input(c_in, shape, B=2):
    idx = S.batch([S.clustered(f"layer/{c_in}/0", shape, 2, 90, 1.6), S.clustered(f"layer/{c_in}/1", shape, 1, 60, 1.2)])
    if shape[0] % 2 == 0:                                   # an even depth: a few sites on the last plane as well
        last = np.asarray([[0, shape[0] - 1, 3, 4], [0, shape[0] - 1, 3, 5], [1, shape[0] - 1, 7, 7]], np.int32)
        idx = np.concatenate([idx, last[~np.isin(S.keys_of(last, B, shape), S.keys_of(idx, B, shape))]])
    return idx, S.synth.uniform(S.SEED, f"trlayer/{c_in}/x", (idx.shape[0], c_in), 0.0, 2.0).astype(np.float32)


def _gpu_layer(feats, idx, B, shape, w, b, kernel, stride, padding, subm, cot, capacity=None, n=None, mw=0, dy_dead=None):
    """train_forward + backward of one layer under the dense cotangent -> {"y" dense, "dx" rows or None, "dW", "db"} on the
    host, and the output tensor. dy_dead: what the cotangent's rows behind the count hold"""
    conv = conv_module(w, b, kernel, stride, padding, subm).train()
    x = tensor(feats, idx, B, shape, capacity=capacity, n=n)
    need_dx = feats.shape[1] >= 16
    x.features.requires_grad_(need_dx)
    out = conv.train_forward(x, max_workgroups=mw)
    i = out.indices.long()
    live = torch.arange(out.capacity, device=i.device) < (out.capacity if out.n is None else out.n)
    i = torch.where(live[:, None], i, torch.zeros_like(i))
    dy = _dev(np.asarray(cot, np.float32))[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]].contiguous()       # rows of the dense cotangent
    if dy_dead is not None:
        dy = torch.where(live[:, None], dy, torch.full_like(dy, dy_dead))
    out.features.backward(dy)
    res = {"y": out.dense().detach().cpu().numpy(), "dx": x.features.grad.cpu().numpy() if need_dx else None,
           "dW": conv.weight.grad.cpu().numpy().reshape(-1, w.shape[4]), "db": None if b is None else conv.bias.grad.cpu().numpy()}
    return res, out


@functools.lru_cache(maxsize=None)
def _layer_truth(c_in, c_out, form, shape=LAYER_GRID):
    kernel, stride, padding, subm = FORMS[form]
    B = 2
    idx, feats = _layer_input(c_in, shape)
    w, b, _ = S.layer_weights(f"trlayer/{c_in}-{c_out}/{form}", kernel, c_in, c_out, True, False)
    osh = shape if subm else S.out_shape(shape, kernel, stride, padding)
    cot = T.cotangent(f"layer/{c_in}-{c_out}/{form}", (B, c_out, *osh))
    args = (feats, idx, shape, w, b, kernel, stride, padding, subm, cot)
    truth = T.layer_train(T.DenseT(B), *args, input_grad=c_in >= 16)
    f32 = T.layer_train(T.DenseT(B, torch.float32), *args, input_grad=c_in >= 16)
    return args, B, truth, f32


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_single_layers_against_float64(pair, form):
    c_in, c_out = pair
    (feats, idx, shape, w, b, kernel, stride, padding, subm, cot), B, truth, f32 = _layer_truth(c_in, c_out, form)
    some_inactive(truth["y"], form)
    got, _ = _gpu_layer(feats, idx, B, shape, w, b, kernel, stride, padding, subm, cot)
    _hold(f"layer/{c_in}-{c_out}/{form}/y", S.rows_of(got["y"]), S.rows_of(f32["y"]), S.rows_of(truth["y"]), S.BARS)
    for k in ("dx", "dW", "db"):
        if truth[k] is None:
            assert got[k] is None and c_in < 16
            continue
        assert got[k].shape == truth[k].shape and np.abs(truth[k]).max() > 0
        _hold(f"layer/{c_in}-{c_out}/{form}/{k}", got[k], f32[k], truth[k])
    if form != "subm":                                      # every tap is exercised
        t = S.table(S.downsample(idx, B, shape, kernel, stride, padding)[0], idx, B, shape, S.out_shape(shape, kernel, stride, padding),
                    kernel, stride, padding)
        assert (t >= 0).any(1).all()


def test_even_depth_rows_without_an_output_site_get_a_zero_gradient():
    shape = (12, 13, 15)                                    # (3,1,1)/(2,1,1): depth 12 -> 5, plane 11 feeds no output site
    (feats, idx, shape, w, b, kernel, stride, padding, subm, cot), B, truth, f32 = _layer_truth(16, 32, "k311s211", shape)
    orphan = idx[:, 1] == shape[0] - 1
    assert orphan.any() and not orphan.all() and _plus_zero(truth["dx"][orphan])
    got, _ = _gpu_layer(feats, idx, B, shape, w, b, kernel, stride, padding, subm, cot)
    assert _plus_zero(got["dx"][orphan])
    for k in ("dx", "dW", "db"):
        _hold(f"layer/even_depth/{k}", got[k], f32[k], truth[k])


def test_dead_rows_change_nothing():
    (feats, idx, shape, w, b, kernel, stride, padding, subm, cot), B, _, _ = _layer_truth(16, 32, "k3s2p1")
    n = idx.shape[0]
    clean, _ = _gpu_layer(feats, idx, B, shape, w, b, kernel, stride, padding, subm, cot)
    # capacity above n: the rows behind hold NaN features, sentinel indices and a NaN cotangent
    dead, out = _gpu_layer(feats, idx, B, shape, w, b, kernel, stride, padding, subm, cot, capacity=n + 37, n=n, dy_dead=float("nan"))
    assert int(out.status.item()) == 0
    for k in ("dW", "db"):
        assert np.array_equal(clean[k].view(np.uint32), dead[k].view(np.uint32)), k
    assert np.array_equal(clean["dx"].view(np.uint32), dead["dx"][:n].view(np.uint32)) and _plus_zero(dead["dx"][n:])
    # a submanifold block with its BatchNorms in train mode: no statistic and no gradient sees the dead rows
    res = []
    for cap in (None, n + 37):
        blk = _block(16)
        x = tensor(feats, idx, B, shape, capacity=cap, n=None if cap is None else n)
        x.features.requires_grad_(True)
        y = blk.train_forward(x)
        g = torch.ones_like(y.features)
        if cap is not None:
            g[n:] = float("nan")
            assert _plus_zero(y.features[n:].detach().cpu().numpy())
        y.features.backward(g)
        res.append({**{k: p.grad.cpu().numpy() for k, p in blk.named_parameters()}, "x": x.features.grad.cpu().numpy(),
                    **{k: v.cpu().numpy() for k, v in blk.named_buffers() if "running" in k}})
    a, d = res
    assert _plus_zero(d["x"][n:])
    d["x"] = d["x"][:n]
    scale = max(np.abs(v).max() for k, v in a.items() if k.endswith("weight"))
    for k in a:
        assert np.isfinite(d[k]).all(), k
        # the same fp32 sums over the same live values and exact zeros; only the order of a sum may differ
        ref = scale if T.zero_by_batchnorm(k) else np.abs(a[k]).max()
        assert np.abs(a[k] - d[k]).max() <= 1e-4 * ref, k


def _block(c, sd=None):
    blk = sparse.SparseBasicBlock(c, c, norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.01), indice_key="b")
    blk.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in (sd or T.block_weights(c)).items()}, strict=False)
    return blk.cuda().train()


# ------------------------------------------------------------------------------------- the K-slice seam, the bits
@functools.lru_cache(maxsize=None)
def _seam_case():
    B, shape = 1, (9, 17, 19)
    idx = _subset("seam", 2 * hip.SP_WGRAD_SLICE + 252, B, shape)
    feats = S.synth.uniform(S.SEED, "seam/x", (idx.shape[0], 16), 0.0, 2.0).astype(np.float32)
    w, b, _ = S.layer_weights("seam/16-16", (3, 3, 3), 16, 16, True, False)
    cot = T.cotangent("seam", (B, 16, *shape))
    return (feats, idx, shape, w, b, (3, 3, 3), (1, 1, 1), (1, 1, 1), True, cot), B


def test_k_slice_seam():
    args, B = _seam_case()
    assert args[1].shape[0] > 2 * hip.SP_WGRAD_SLICE
    truth, f32 = T.layer_train(T.DenseT(B), *args), T.layer_train(T.DenseT(B, torch.float32), *args)
    got, _ = _gpu_layer(args[0], args[1], B, *args[2:])
    for k in ("dx", "dW", "db"):
        _hold(f"seam/{k}", got[k], f32[k], truth[k])


@pytest.mark.parametrize("case", ("seam", "64-128/k3s2p1", "128-128/k311s211"))
def test_bits_do_not_depend_on_the_grid_or_the_run(case):
    if case == "seam":
        args, B = _seam_case()
    else:
        pair, form = case.split("/")
        args, B, _, _ = _layer_truth(*(int(v) for v in pair.split("-")), form)
    ref = None
    for mw in (0, 0, 1, 3):
        got, _ = _gpu_layer(args[0], args[1], B, *args[2:], mw=mw)
        if ref is None:
            ref = got
        for k in ("y", "dx", "dW", "db"):
            assert np.array_equal(ref[k].view(np.uint32), got[k].view(np.uint32)), (case, mw, k)


# ------------------------------------------------------------------------------------- the block and the backbone
def test_block_train_forward_against_float64():
    B, shape = 2, LAYER_GRID
    idx, feats = _layer_input(32, shape)
    sd = T.block_weights(32)
    cot = T.cotangent("block", (B, 32, *shape))
    truth, f32 = T.block_train(T.DenseT(B), sd, feats, idx, shape, cot), T.block_train(T.DenseT(B, torch.float32), sd, feats, idx, shape, cot)
    blk = _block(32, sd)
    x = tensor(feats, idx, B, shape, capacity=idx.shape[0] + 37, n=idx.shape[0])
    x.features.requires_grad_(True)
    y = blk.train_forward(x)
    d = y.dense()
    (d * _dev(cot.astype(np.float32))).sum().backward()
    _hold("block/y", S.rows_of(d.detach().cpu().numpy()), S.rows_of(f32[0]), S.rows_of(truth[0]))
    got = {k: p.grad.cpu().numpy() for k, p in blk.named_parameters()}
    got["x"] = x.features.grad.cpu().numpy()[:idx.shape[0]]
    scale = max(np.abs(v).max() for k, v in truth[1].items() if k.endswith("weight"))
    for k in sorted(truth[1]):
        if T.zero_by_batchnorm(k):
            assert np.abs(got[k]).max() <= 1e-4 * scale, k
        else:
            _hold(f"block/grad/{k}", got[k], f32[1][k], truth[1][k])
    for k in sorted(truth[2]):
        _hold(f"block/{k}", dict(blk.named_buffers())[k].cpu().numpy(), f32[2][k], truth[2][k])
    assert int(blk.bn1.num_batches_tracked) == int(blk.bn2.num_batches_tracked) == 1


@functools.lru_cache(maxsize=None)
def _backbone_truth(train=True):
    feats, idx, B, shape = T.train_case(5)
    sd = S.backbone_weights(5)
    cot = T.cotangent("bev", (B, 128, 4, 5)) if train else None
    return (feats, idx, B, shape, sd, cot, T.backbone_train(T.DenseT(B), sd, feats, idx, shape, cot, train),
            T.backbone_train(T.DenseT(B, torch.float32), sd, feats, idx, shape, cot, train))


def _hold_backbone(prefix, m, bev, levels, truth, f32, bars=None):
    out, grads, stats = truth
    _hold(f"{prefix}/bev", S.rows_of(bev.detach().cpu().numpy()), S.rows_of(f32[0]["bev"]), S.rows_of(out["bev"]), bars)
    for k in S.LEVELS:
        _hold(f"{prefix}/{k}", S.rows_of(levels[k].dense().detach().cpu().numpy()), S.rows_of(f32[0][k]), S.rows_of(out[k]), bars)
    params = dict(m.named_parameters())
    scale = max([np.abs(v).max() for k, v in grads.items() if k.endswith("weight")] + [0.0])
    for k in sorted(grads):
        assert params[k].grad is not None and bool(torch.isfinite(params[k].grad).all()), k
        if T.zero_by_batchnorm(k):
            assert float(params[k].grad.abs().max()) <= 1e-4 * scale, k
        else:
            _hold(f"{prefix}/grad/{k}", params[k].grad.cpu().numpy(), f32[1][k], grads[k], bars)
    buffers = dict(m.named_buffers())
    for k in sorted(stats):
        _hold(f"{prefix}/{k}", buffers[k].cpu().numpy(), f32[2][k], stats[k], bars)


def test_backbone_train_forward_and_backward_against_float64():
    feats, idx, B, shape, sd, cot, truth, f32 = _backbone_truth()
    for k in S.LEVELS + ("bev",):
        for b in (0, 1):
            some_inactive(truth[0][k][b:b + 1], (k, b))
    assert int((np.abs(truth[0]["bev"]).max(1) > 0).sum()) >= 16
    n = idx.shape[0]
    voxel_shape = [shape[2], shape[1], shape[0] - 1]
    pad = 37                                                # capacity above the count: NaN features, sentinel coordinates
    df = _dev(np.concatenate([feats, np.full((pad, feats.shape[1]), np.nan, np.float32)]))
    di = _dev(np.concatenate([idx, np.full((pad, 4), SENTINEL, np.int32)]))
    dn = torch.tensor([n], dtype=torch.int64).cuda()
    dcot = _dev(cot.astype(np.float32))
    warm = backbone_module(5).train()
    bev, _ = warm.train_forward(df, di, B, voxel_shape, n_voxels=dn)
    (bev * dcot).sum().backward()
    m = backbone_module(5).train()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                 # nothing synchronises, in either direction
    try:
        bev, levels = m.train_forward(df, di, B, voxel_shape, n_voxels=dn)
        (bev * dcot).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(m.last_status.item()) == 0 and bev.shape == (4, 128, 4, 5) and list(levels) == list(S.LEVELS)
    counts = [n] + [int(levels[k].n.item()) for k in ("conv2", "conv3", "conv4")]
    assert tuple(counts) == T.TRAIN_SITES[:4]
    _hold_backbone("backbone/train", m, bev, levels, truth, f32)
    assert all(int(v) == 8 for k, v in m.named_buffers() if k.endswith("num_batches_tracked"))
    for k, p in warm.named_parameters():                    # the same bits from run to run
        assert torch.equal(p.grad, dict(m.named_parameters())[k].grad), k
    with pytest.raises(RuntimeError, match="eval-mode"):    # forward() in train mode stays refused
        m(df, di, B, voxel_shape)


def test_train_forward_with_frozen_batchnorm_is_the_eval_forward():
    feats, idx, B, shape, sd, _, truth, f32 = _backbone_truth(False)
    voxel_shape = [shape[2], shape[1], shape[0] - 1]
    m = backbone_module(5)                                  # eval mode: every BatchNorm uses its running statistics
    bev, levels = m.train_forward(_dev(feats), _dev(idx), B, voxel_shape)
    with torch.no_grad():
        bev0, levels0 = m(_dev(feats), _dev(idx), B, voxel_shape)
    assert bev.requires_grad and bev.shape == bev0.shape
    for row, got in (("train_forward", bev), ("forward", bev0)):
        _hold(f"backbone/eval/{row}/bev", S.rows_of(got.detach().cpu().numpy()), S.rows_of(f32[0]["bev"]), S.rows_of(truth[0]["bev"]), S.BARS)
    assert all(int(v) == 7 for k, v in m.named_buffers() if k.endswith("num_batches_tracked"))
    bev.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


# ------------------------------------------------------------------------------------- the detector's first-stage loss
def test_first_stage_loss_reaches_every_parameter():
    import importlib
    V = importlib.import_module("test_gpu_voxelnet")
    detector, pillars = V.detector, V.pillars
    center_loss = importlib.import_module("3dal_pytorch_amd.center_loss")
    pts, off = V.sweep()
    r = pillars.voxelize(_dev(pts), off, V.VOXEL, V.RANGE, 5, 4000)
    voxels, coords, num, nv = r.finish()
    gt = np.zeros((2, 4, 10), np.float32)
    gt[0, 0] = [-1.5, 1.0, 0.0, 1.8, 4.2, 1.6, 0.3, 0, 0, 1]
    gt[0, 1] = [2.0, -2.5, 0.2, 0.7, 0.8, 1.7, -1.0, 0, 0, 2]
    gt[1, 0] = [0.5, 2.5, -0.1, 0.6, 1.7, 1.5, 2.0, 0, 0, 3]
    targets = center_loss.center_targets(_dev(gt), [3], V.RANGE, V.VOXEL, 8, (2, 2))
    example = dict(voxels=voxels, coordinates=coords, num_points=num, num_voxels=nv, shape=[V.GRID] * 2, **targets)
    sd = V.checkpoint()

    m = detector.VoxelNet(**V.MODEL, **V.KW)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    kept, inner = {}, m.backbone.train_forward

    def spy(feat, *args, **kw):                             # keep the backbone's input and outputs, and d loss / d bev
        bev, levels = inner(feat, *args, **kw)
        bev.retain_grad()
        kept.update(feat=feat, bev=bev, levels=levels)
        return bev, levels

    m.backbone.train_forward = spy
    out = m.first_stage_loss(example)
    assert set(out) >= {"loss", "hm_loss", "loc_loss", "loc_loss_elem", "num_positive"} and len(out["loss"]) == 1
    sum(out["loss"]).backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert float(sum(out["loss"])) > 0 and float(out["num_positive"][0]) > 0
    # d loss / d bev as the cotangent: the backbone's gradients against the float64 restatement
    feat, bev, levels = kept["feat"], kept["bev"], kept["levels"]
    cot = bev.grad.cpu().numpy().astype(np.float64)
    assert np.abs(cot).max() > 0
    bsd = S.backbone_weights(5)
    args = (bsd, feat.cpu().numpy(), coords.cpu().numpy(), (V.GRID[2] + 1, V.GRID[1], V.GRID[0]), cot)
    truth, f32 = T.backbone_train(T.DenseT(2), *args), T.backbone_train(T.DenseT(2, torch.float32), *args)
    _hold_backbone("first_stage", m.backbone, bev, levels, truth, f32)
