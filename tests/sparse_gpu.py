"""What tests/test_gpu_sparse.py, tests/test_gpu_sparse_edges.py and tests/test_gpu_voxelnet.py share: sparse tensors and single layers on the device,
the bookkeeping walked level by level next to sparse_ref's rulebook, references computed once, and the record of every
figure held under DAL3_SPARSE_RECORD=<path> (how profiles/sparse_measured.json is made: run both files in one session)."""
import functools
import importlib
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import sparse_ref as S

hip = importlib.import_module("3dal_pytorch_amd._hip")
sparse = importlib.import_module("3dal_pytorch_amd.sparse")
_RECORD = {}
SENTINEL = -7
GUARD = 64                                      # rows either side of a guarded buffer


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """imported by both test files: each writes all the figures held so far when its last test is done"""
    yield
    path = os.environ.get("DAL3_SPARSE_RECORD")
    if path and _RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _hold(row, got, f32, truth):
    """each measure <= bar x the fp32 yardstick's own error against the truth, dead channels +0"""
    ratio, m, y = S.ratios(got, f32, truth)
    _RECORD[row] = {"measured": {k: m[k] for k in S.MEASURES}, "yardstick": {k: y[k] for k in S.MEASURES}, "ratio": ratio}
    for k in S.MEASURES:
        print(f"{row:40s} {k:9s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:7.2f}  bar {S.BARS[k]:g}")
    assert m["dead_ok"]
    bad = [(k, m[k], ratio[k]) for k in S.MEASURES if ratio[k] > S.BARS[k]]
    assert not bad, (row, bad)


def some_inactive(dense, what):
    """the truth has both active and inactive cells in every sample that has any: a saturated level tests no mask"""
    act = np.abs(np.asarray(dense)).max(1) > 0
    assert act.any() and not act.all(), f"{what}: {int(act.sum())} of {act.size} cells are active"


def tensor(feats, idx, B, shape, capacity=None, n=None):
    """a SparseConvTensor on the device; capacity > rows pads with sentinel rows, n: the device count"""
    feats, idx = np.asarray(feats, np.float32), np.asarray(idx, np.int32).reshape(-1, 4)
    if capacity is not None and capacity > idx.shape[0]:
        pad = capacity - idx.shape[0]
        feats = np.concatenate([feats, np.full((pad, feats.shape[1]), np.nan, np.float32)])
        idx = np.concatenate([idx, np.full((pad, 4), SENTINEL, np.int32)])
    return sparse.SparseConvTensor(_dev(feats), _dev(idx), shape, B, n=None if n is None else torch.tensor([n], dtype=torch.int64).cuda())


def conv_module(w, b, kernel, stride, padding, subm, key=None):
    cls = sparse.SubMConv3d if subm else sparse.SparseConv3d
    m = cls(w.shape[3], w.shape[4], kernel, stride, padding, bias=b is not None, indice_key=key)
    m.weight.data = torch.from_numpy(np.ascontiguousarray(w))
    if b is not None:
        m.bias.data = torch.from_numpy(b)
    return m.cuda().eval()


def bn_module(bn, eps=S.EPS):
    if bn is None:
        return None
    m = nn.BatchNorm1d(len(bn[0]), eps=eps)
    for t, v in zip((m.weight, m.bias, m.running_mean, m.running_var), bn):
        t.data = torch.from_numpy(np.asarray(v))
    return m.cuda().eval()


@torch.no_grad()
def run_layer(x, w, b, bn, kernel, stride, padding, subm, relu, residual=False, canvas=False, **kw):
    """fold + pack + the bookkeeping + one dal3_sp_conv launch -> the dense output (B, c_out, D', H', W') on the host (with
    canvas=True the BEV store, reshaped back), and the output tensor (None with a canvas)"""
    conv = conv_module(w, b, kernel, stride, padding, subm)
    packed = sparse.pack_layer(conv, bn_module(bn))
    out = conv.run(x, packed, relu=relu, residual=x.features if residual else None, canvas=canvas, **kw)
    if canvas:
        D = sparse.out_shape(x.spatial_shape, conv.kernel_size, conv.stride, conv.padding)[0]
        bev = out.cpu().numpy()
        return bev.reshape(bev.shape[0], -1, D, *bev.shape[2:]), None
    return out.dense().cpu().numpy(), out


def windows(shape):
    """the strided stems that still fit, level by level -> [(name, kernel, stride, padding, out shape)]"""
    out = []
    for name, _, kernel, stride, padding in S.STEMS[1:]:
        if any(n + 2 * p < k for n, k, p in zip(shape, kernel, padding)):
            break
        shape = S.out_shape(shape, kernel, stride, padding)
        out.append((name, kernel, stride, padding, shape))
    return out


def book_ref(idx, B, shape, table=S.table):
    """every level's integers by sparse_ref: [(name, indices, shape, the 27-tap table, the strided table or None)].
    table: S.table, or S.table_sorted for levels of thousands of sites"""
    idx = np.asarray(idx, np.int32).reshape(-1, 4)
    levels = [("res0", idx, tuple(shape), table(idx, idx, B, shape, shape, (3, 3, 3), (1, 1, 1), (1, 1, 1)), None)]
    for name, kernel, stride, padding, osh in windows(shape):
        o, _ = S.downsample(idx, B, shape, kernel, stride, padding)
        down = table(o, idx, B, shape, osh, kernel, stride, padding)
        levels.append((name, o, osh, table(o, o, B, osh, osh, (3, 3, 3), (1, 1, 1), (1, 1, 1)), down))
        idx, shape = o, osh
    return levels


class Guarded:
    """a device buffer of `rows` rows with GUARD sentinel rows either side"""

    def __init__(self, rows, cols, dtype=torch.int32):
        self.all = torch.full((rows + 2 * GUARD, cols) if cols else (rows + 2 * GUARD,), SENTINEL, dtype=dtype).cuda()
        self.view = self.all[GUARD:GUARD + rows]

    def intact(self):
        return bool((self.all[:GUARD] == SENTINEL).all() and (self.all[GUARD + self.view.shape[0]:] == SENTINEL).all())


@torch.no_grad()
def book_gpu(x, caps=None, max_workgroups=0, inverse=None):
    """the same walk on the device through sparse.py's bookkeeping, every output in a guarded, sentinel-filled buffer ->
    [(name, indices, n, shape, table27, strided table or None, capacity)] as host arrays, and whether every guard is intact.
    inverse: a list that takes every strided level's transposed table, (name, (taps, input capacity) host array), built in a
    guarded buffer too"""
    caps, bufs = caps or {}, []
    levels = [("res0", x.indices.cpu().numpy(), None if x.n is None else int(x.n.item()), x.spatial_shape,
               sparse.subm_table(x, None, max_workgroups).cpu().numpy(), None, x.capacity)]
    for name, kernel, stride, padding, osh in windows(x.spatial_shape):
        cap = caps.get(name, sparse.safe_capacity(x.capacity, x.batch_size, x.spatial_shape, kernel, stride, padding))
        gi, gk = Guarded(cap, 4), Guarded(cap, 0)
        indices, keys, n_out, cap, shape = sparse.downsample(x, kernel, stride, padding, cap, max_workgroups, gi.view, gk.view)
        assert shape == osh
        taps = int(np.prod(kernel))
        gt = Guarded(taps * cap, 0)
        down = sparse.neighbour_table(x, indices, n_out, cap, shape, kernel, stride, padding, max_workgroups, gt.view.view(taps, cap))
        y = sparse.SparseConvTensor(torch.zeros((cap, 1), dtype=torch.float32).cuda(), indices, shape, x.batch_size, n_out, x.status)
        y.sorted = (keys, None)
        g27 = Guarded(27 * cap, 0)
        t27 = sparse.neighbour_table(y, indices, n_out, cap, shape, (3, 3, 3), (1, 1, 1), (1, 1, 1), max_workgroups, g27.view.view(27, cap))
        bufs += [gi, gk, gt, g27]
        if inverse is not None:
            gv = Guarded(taps * x.capacity, 0)
            inv = sparse.transposed_table(x, keys, n_out, cap, shape, kernel, stride, padding, max_workgroups, gv.view.view(taps, x.capacity))
            inverse.append((name, inv.cpu().numpy()))
            bufs.append(gv)
        levels.append((name, indices.cpu().numpy(), int(n_out.item()), shape, t27.cpu().numpy(), down.cpu().numpy(), cap))
        x = y
    return levels, all(b.intact() for b in bufs)


def same_book(got, want):
    """indices, counts and tables of every level are the reference's; rows beyond a count keep the sentinel"""
    assert [g[0] for g in got] == [w[0] for w in want]
    for (name, gi, gn, gshape, g27, gdown, cap), (_, wi, wshape, w27, wdown) in zip(got, want):
        n = wi.shape[0]
        assert tuple(gshape) == tuple(wshape), name
        assert gn is None or gn == n, (name, gn, n)
        assert np.array_equal(gi[:n], wi), name
        assert np.array_equal(g27[:, :n], w27), name
        if name != "res0":
            assert np.array_equal(gdown[:, :n], wdown), name
            assert (gi[n:] == SENTINEL).all() and (g27[:, n:] == SENTINEL).all() and (gdown[:, n:] == SENTINEL).all(), name


def backbone_module(c_in, device="cuda"):
    m = sparse.SpMiddleResNetFHD(num_input_features=c_in, ds_factor=8)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in S.backbone_weights(c_in).items()}, strict=True)
    return m.to(device).eval()


@functools.lru_cache(maxsize=None)
def backbone_truth(c_in, poison=False):
    """the seeded backbone case -> (feats, idx, B, shape, float64 truth, torch-CPU fp32 yardstick), computed once and shared
    (read-only). poison: a NaN and an Inf in one voxel's features: the corner voxel (0, 0, 0) of the two-voxel sample, so that
    the finite rest keeps the clustered sample's few hundred sites, which the per-channel measures presuppose (sparse_ref.BARS)"""
    feats, idx, B, shape = S.backbone_case(c_in)
    if poison:
        feats = feats.copy()
        assert idx[-2].tolist() == [2, 0, 0, 0]
        feats[-2, 1], feats[-2, 0] = np.nan, np.inf
    sd = S.backbone_weights(c_in)
    truth = S.backbone(S.Dense(B), sd, feats, idx, shape)
    f32 = S.backbone(S.Dense(B, torch.float32), sd, feats, idx, shape)
    for d in (truth, f32):
        for a in d.values():
            a.setflags(write=False)
    return feats, idx, B, shape, truth, f32
