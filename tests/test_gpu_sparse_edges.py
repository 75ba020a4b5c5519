"""The sparse middle's integer bookkeeping (dal3_sp_sort, dal3_sp_downsample, dal3_sp_table, dal3_sp_table_transposed)
against sparse_ref's rulebook, exactly, where tests/test_gpu_sparse.py does not go: every radix pass count up to the
production grid's 29-bit keys, sorts over several chunks with runs of equal keys across the tile and chunk seams, every
per-axis window the entry points admit, and every relation of a count to a capacity. The cases and what each one hits are
tests/sparse_book_cases.py's, asserted on the CPU by tests/test_sparse_book_cases_cpu.py. One submanifold and one strided
layer on the production grid are held to the float64 rulebook under sparse_ref.BARS, the fp32 rulebook as the yardstick."""
import numpy as np
import pytest
import torch

import sparse_book_cases as K
import sparse_ref as S
import sparse_train_ref as T
from sparse_gpu import (SENTINEL, Guarded, _hold, _record_file, bn_module, book_gpu, book_ref, conv_module, hip, same_book, sparse, tensor,  # noqa: F401
                        windows)

pytestmark = pytest.mark.gpu


def _inverse_ref(want, B):
    """every strided level's transposed table from book_ref's levels"""
    out = []
    for (_, idx, shape, _, _), (name, o, osh, _, _), (_, kernel, stride, padding, _) in zip(want, want[1:], windows(want[0][2])):
        out.append((name, T.inverse_table(idx, o, B, shape, osh, kernel, stride, padding)))
    return out


def _same_inverse(inverse, inv_want, n_in, got):
    """the transposed tables are the reference's; columns behind the input's count keep the sentinel"""
    assert [i[0] for i in inverse] == [w[0] for w in inv_want]
    for (name, inv), (_, winv), level in zip(inverse, inv_want, got[1:]):
        assert winv.shape[1] == n_in and np.array_equal(inv[:, :n_in], winv), name
        assert (inv[:, n_in:] == SENTINEL).all(), name
        n_in = level[2]


def _walk_exactly(idx, B, shape, capacity, mws=(0, 1, 3)):
    """indices, counts, the 27-tap, strided and transposed tables of every level are the rulebook's, behind intact guards,
    with status 0 and the same bytes for every max_workgroups"""
    n = idx.shape[0]
    want = book_ref(idx, B, shape, S.table_sorted)
    inv_want = _inverse_ref(want, B)
    ref = None
    for mw in mws:
        x = tensor(np.zeros((n, 1), np.float32), idx, B, shape, capacity=capacity, n=n)
        inverse = []
        got, intact = book_gpu(x, max_workgroups=mw, inverse=inverse)
        assert intact and int(x.status.item()) == 0
        assert len(got) == len(want) == len(K.levels(shape))
        same_book(got, want)
        _same_inverse(inverse, inv_want, n, got)
        flat = [got[0][4][:, :n]] + [a for g in got[1:] for a in (g[1], g[4], g[5])] + [i[1] for i in inverse]
        if ref is None:
            ref = flat
        else:
            assert all(np.array_equal(a, b) for a, b in zip(flat, ref)), f"max_workgroups {mw} changes the bytes"
    return want


@pytest.mark.parametrize("name", sorted(K.WIDTH_GRIDS))
def test_every_key_width(name):
    """1, 2, 3 and 4 radix passes at the sort and at the downsamples; `largest` is the widest key sp_grid_ok admits and
    `waymo` the detector's grid at B = 4 (4, 4, 3, 3, 3 passes)"""
    idx, B, shape = K.width_case(name)
    want = _walk_exactly(idx, B, shape, idx.shape[0] + K.MARGIN)
    assert all(w[1].shape[0] > 0 for w in want)


@pytest.mark.parametrize("grid,capacity", K.LENGTH_CASES)
def test_every_chunk_and_scan_seam(grid, capacity):
    """sort lengths of 4095 .. 8193 entries, candidate lists of 4088 .. 262152, on a 2-pass and on a 3-pass grid"""
    idx, B, shape, cap = K.length_case(grid, capacity)
    _walk_exactly(idx, B, shape, cap, mws=(0, 3) if capacity == 32769 else (0, 1, 3))


# ------------------------------------------------------------------------------------- one arbitrary window
@torch.no_grad()
def window_gpu(x, kernel, stride, padding, capacity=None, max_workgroups=0):
    """sparse.downsample -> neighbour_table -> transposed_table on one window, every output in a guarded buffer ->
    ({indices, keys, n, shape, table, inverse, capacity} as host arrays, guards intact)"""
    cap = sparse.safe_capacity(x.capacity, x.batch_size, x.spatial_shape, kernel, stride, padding) if capacity is None else capacity
    gi, gk = Guarded(cap, 4), Guarded(cap, 0)
    indices, keys, n_out, cap, shape = sparse.downsample(x, kernel, stride, padding, cap, max_workgroups, gi.view, gk.view)
    taps = int(np.prod(kernel))
    gt, gv = Guarded(taps * cap, 0), Guarded(taps * x.capacity, 0)
    table = sparse.neighbour_table(x, indices, n_out, cap, shape, kernel, stride, padding, max_workgroups, gt.view.view(taps, cap))
    inv = sparse.transposed_table(x, keys, n_out, cap, shape, kernel, stride, padding, max_workgroups, gv.view.view(taps, x.capacity))
    out = dict(indices=indices.cpu().numpy(), keys=keys.cpu().numpy(), n=int(n_out.item()), shape=shape, table=table.cpu().numpy(),
               inverse=inv.cpu().numpy(), capacity=cap)
    return out, all(g.intact() for g in (gi, gk, gt, gv))


@pytest.mark.parametrize("case", range(len(K.window_cases())), ids=lambda c: "k{}{}{}-s{}{}{}-p{}{}{}".format(*sum(K.window_cases()[c], ())))
def test_every_admitted_window(case):
    """kernel 1 .. 3, stride 1 .. 3, padding 0 .. 2 per axis, three different per-axis windows a case: k < s (inputs that feed
    no output) and p >= k (outputs that see padding only) among them"""
    kernel, stride, padding = K.window_cases()[case]
    idx, B, shape = K.window_sites()
    n = idx.shape[0]
    o, osh = S.downsample(idx, B, shape, kernel, stride, padding)
    m = o.shape[0]
    want_table = S.table_sorted(o, idx, B, shape, osh, kernel, stride, padding)
    want_inv = T.inverse_table(idx, o, B, shape, osh, kernel, stride, padding)
    assert m > 0 and (want_table >= 0).any()
    ref = None
    for mw in (0, 1, 3):
        x = tensor(np.zeros((n, 1), np.float32), idx, B, shape, capacity=n + K.MARGIN, n=n)
        got, intact = window_gpu(x, kernel, stride, padding, max_workgroups=mw)
        assert intact and int(x.status.item()) == 0
        assert got["shape"] == osh and got["n"] == m and got["capacity"] >= m
        assert np.array_equal(got["indices"][:m], o) and np.array_equal(got["keys"][:m], S.keys_of(o, B, osh))
        assert np.array_equal(got["table"][:, :m], want_table) and np.array_equal(got["inverse"][:, :n], want_inv)
        for k in ("indices", "keys"):
            assert (got[k][m:] == SENTINEL).all(), k
        assert (got["table"][:, m:] == SENTINEL).all() and (got["inverse"][:, n:] == SENTINEL).all()
        flat = [got[k] for k in ("indices", "keys", "table", "inverse")]
        if ref is None:
            ref = flat
        else:
            assert all(np.array_equal(a, b) for a, b in zip(flat, ref)), f"max_workgroups {mw} changes the bytes"


# ------------------------------------------------------------------------------------- counts and capacities
def _in_bounds(levels):
    for _, gi, gn, gshape, g27, gdown, c in levels:
        assert 0 <= gn <= c and (g27[:, :gn] < gn).all() and (g27[:, :gn] >= -1).all()
        assert (gi[:gn] >= 0).all() and (gi[:gn, 1:] < np.asarray(gshape)).all()


def _count_truth():
    idx, B, shape = K.count_case()
    return idx, B, shape, book_ref(idx, B, shape)


def test_a_capacity_equal_to_the_count_holds_every_site():
    idx, B, shape, want = _count_truth()
    x = tensor(np.zeros((300, 1), np.float32), idx, B, shape)
    got, intact = book_gpu(x, caps={w[0]: w[1].shape[0] for w in want[1:]})
    assert intact and int(x.status.item()) == 0
    same_book(got, want)
    assert [g[6] for g in got[1:]] == [w[1].shape[0] for w in want[1:]]


def test_a_capacity_one_below_the_count_drops_the_last_site_by_key():
    idx, B, shape, want = _count_truth()
    o, osh = want[1][1], want[1][2]
    cap = o.shape[0] - 1
    x = tensor(np.zeros((300, 1), np.float32), idx, B, shape)
    got, intact = book_gpu(x, caps={"conv2": cap})
    assert intact and int(x.status.item()) == hip.SP_OVERFLOW
    name, gi, gn, _, g27, gdown, c = got[1]
    assert (name, gn, c) == ("conv2", cap, cap) and np.array_equal(gi, o[:cap])               # the first sites by key survive
    assert np.array_equal(g27, S.table_sorted(o[:cap], o[:cap], B, osh, osh, (3, 3, 3), (1, 1, 1), (1, 1, 1)))
    assert np.array_equal(gdown, S.table_sorted(o[:cap], idx, B, shape, osh, (3, 3, 3), (2, 2, 2), (1, 1, 1)))
    _in_bounds(got[2:])


def test_a_capacity_of_zero_writes_nothing():
    idx, B, shape, want = _count_truth()
    for n, status in ((None, hip.SP_OVERFLOW), (0, 0)):                     # the bit if and only if there was a site
        x = tensor(np.zeros((300, 1), np.float32), idx, B, shape, n=n)
        got, intact = book_gpu(x, caps={"conv2": 0})
        assert intact and int(x.status.item()) == status
        assert [(g[2], g[6]) for g in got[1:]] == [(0, 0)] * 4
        assert all(g[1].shape == (0, 4) and g[4].size == 0 and g[5].size == 0 for g in got[1:])


@pytest.mark.parametrize("count", (0, -3))
def test_a_device_count_of_zero_or_below_empties_every_level(count):
    idx, B, shape, want = _count_truth()
    assert K.live(count, 300 + K.MARGIN) == 0
    x = tensor(np.zeros((300, 1), np.float32), idx, B, shape, capacity=300 + K.MARGIN, n=count)
    inverse = []
    got, intact = book_gpu(x, inverse=inverse)
    assert intact and int(x.status.item()) == 0
    for _, gi, gn, _, g27, gdown, c in got[1:]:
        assert gn == 0 and c > 0 and (gi == SENTINEL).all() and (g27 == SENTINEL).all() and (gdown == SENTINEL).all()
    assert all((inv == SENTINEL).all() for _, inv in inverse)


def test_a_device_count_above_the_capacity_is_the_capacity():
    idx, B, shape, want = _count_truth()
    assert K.live(305, 300) == 300
    x = tensor(np.zeros((300, 1), np.float32), idx, B, shape, n=300 + 5)
    inverse = []
    got, intact = book_gpu(x, inverse=inverse)
    assert intact and int(x.status.item()) == 0
    assert np.array_equal(got[0][4], want[0][3])
    same_book(got[1:], want[1:])
    _same_inverse(inverse, _inverse_ref(want, B), 300, got)


# ------------------------------------------------------------------------------------- one convolution on wide keys
WIDE = {"subm": ((3, 3, 3), (1, 1, 1), (1, 1, 1), True), "k3s2p1": ((3, 3, 3), (2, 2, 2), (1, 1, 1), False)}


@pytest.mark.parametrize("form", sorted(WIDE))
def test_one_convolution_on_the_production_grid(form):
    """16 -> 32 channels on 4 x (41, 1504, 1504): the rulebook in float64 is the truth and the same rulebook in float32 the
    yardstick (no dense array holds this grid), under sparse_ref.BARS"""
    kernel, stride, padding, subm = WIDE[form]
    idx, B, shape = K.width_case("waymo")
    n = idx.shape[0]
    feats = S.synth.uniform(S.SEED, "wide/x", (n, 16), 0.0, 2.0).astype(np.float32)
    w, b, bn = S.layer_weights(f"wide/{form}", kernel, 16, 32, subm, True)
    args = (feats, idx, shape, w, b, bn, kernel, stride, padding, subm, True)
    truth, oidx, osh = S.layer_rows(S.Rulebook(B, table=S.table_sorted), *args)
    f32, _, _ = S.layer_rows(S.Rulebook(B, dtype=np.float32, table=S.table_sorted), *args)
    assert truth.dtype == np.float64 and f32.dtype == np.float32 and truth.shape == (oidx.shape[0], 32)
    x = tensor(feats, idx, B, shape, capacity=n + K.MARGIN, n=n)
    conv = conv_module(w, b, kernel, stride, padding, subm)
    with torch.no_grad():
        y = conv.run(x, sparse.pack_layer(conv, bn_module(bn)), relu=True)
    m = oidx.shape[0]
    assert int(x.status.item()) == 0 and y.spatial_shape == tuple(osh) and int(y.n.item()) == m
    assert np.array_equal(y.indices.cpu().numpy()[:m], oidx)
    got = y.features.cpu().numpy()[:m]
    _hold(f"wide/{form}", got.T[None], f32.T[None], truth.T[None])
