"""The row queue of the fp32 decoder's compacted body on the CPU (tests/dec_queue_model.py): the whole-layer chains of
dconv3 and dconv4 through the mask, the list and the zero pad, and dconv2's chain per group of chunks, give the dense
fmaf chain's bits."""
import numpy as np
import pytest

import dec_queue_model as Q
import dec_sparse_model as M


def _layer(rng, K, n_out=48):
    return rng.standard_normal((n_out, K)).astype(np.float32), rng.standard_normal(n_out).astype(np.float32)


def _activations(rng, K, dead):
    """post-ReLU activations (K, 32 n_tiles): about half of the elements +0; chain position k of tile t is +0 in all 32
    points where dead[t, k], and live in at least one point elsewhere"""
    n_tiles = dead.shape[0]
    a = np.maximum(rng.standard_normal((K, n_tiles * Q.TILE)), 0).astype(np.float32)
    a[:, ::Q.TILE] = np.float32(0.5)
    out = np.zeros_like(a)
    out[Q.chain(K)] = a[Q.chain(K)] * np.repeat(~dead.T, Q.TILE, axis=1)
    return out


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _edge_cases(K, rng):
    """tiles: random p = 0.1 / 0.45 / 0.9, all dead, none dead, only the last chain index, only the first, an odd count"""
    dead = np.ones((8, K), bool)
    for t, p in enumerate((0.1, 0.45, 0.9)):
        dead[t] = rng.random(K) < p
    dead[4] = False
    dead[5, K - 1] = False
    dead[6, 0] = False
    dead[7, rng.permutation(K)[:K // 3 | 1]] = False
    return dead


@pytest.mark.parametrize("K", [256, 128])
def test_whole_layer_queue_reproduces_the_dense_chain(K):
    """dconv3 (K = 256) and dconv4 (K = 128)"""
    rng = np.random.default_rng(K)
    dead = _edge_cases(K, rng)
    w, b = _layer(rng, K)
    act = _activations(rng, K, dead)
    assert np.array_equal(Q.live_rows(act), ~dead)
    got, steps, live = Q.queue_chain(w, b, act)
    assert _same_bits(got, Q.dense_chain(w, b, act))
    assert np.array_equal(live, (~dead).sum(axis=1)) and np.array_equal(steps, (live + 1) // 2)
    assert steps[3] == 0 and steps[4] == K // 2 and steps[5] == 1 and steps[6] == 1


def test_the_list_is_the_live_chain_indices_in_order_and_ends_on_the_row_of_zeros():
    rng = np.random.default_rng(3)
    for p in (0.0, 0.3, 0.97, 1.0):
        mask = rng.random(256) >= p
        lst, cnt = Q.live_list(mask)
        assert cnt == int(mask.sum()) and lst[:cnt].tolist() == np.nonzero(mask)[0].tolist()
        assert (lst[cnt:cnt + Q.LIST_OVER] == Q.ZERO_ROW).all()


def test_chain_order_is_the_dense_layers_order():
    """k-tile, then register, then low half before high half; dconv2's chain is the same map over 16 k-tiles"""
    assert Q.chain(512).tolist() == M.CHAIN.tolist()
    assert Q.chain(64)[:6].tolist() == [0, 4, 1, 5, 2, 6] and Q.chain(64)[32] == 32


def test_nan_and_inf_rows_are_live():
    rng = np.random.default_rng(4)
    dead = np.ones((1, 128), bool)
    act = _activations(rng, 128, dead)
    act[7, 3], act[90, 31] = np.nan, np.inf
    live = Q.live_rows(act)[0]
    ch = Q.chain(128)
    assert sorted(ch[np.nonzero(live)[0]].tolist()) == [7, 90]
    w, b = _layer(rng, 128)
    got, steps, _ = Q.queue_chain(w, b, act)
    assert _same_bits(got, Q.dense_chain(w, b, act)) and steps.tolist() == [1]


@pytest.mark.parametrize("group", [1, 2, 4, 8])
def test_grouped_dconv2_reproduces_the_dense_chain(group):
    """random dead sets; an odd leftover carried across several groups (one live row, then empty groups, then a partner); an
    empty group; a full group; only the last chain index; only the first"""
    rng = np.random.default_rng(10 + group)
    K, span = 512, 32 * group
    dead = np.ones((9, K), bool)
    for t, p in enumerate((0.1, 0.45, 0.9)):
        dead[t] = rng.random(K) < p
    dead[3, 5] = False                                     # waits through the groups in between ...
    dead[3, K - span + 1] = False                          # ... for a partner in the last group
    dead[4] = rng.random(K) < 0.45
    dead[4, span:2 * span] = True                          # an empty group (the second, or the only other one)
    dead[5] = rng.random(K) < 0.45
    dead[5, :span] = False                                 # a full group
    dead[6, K - 1] = False
    dead[7, 0] = False
    for g in range(K // span):                             # every group holds an odd count
        dead[8, g * span + rng.permutation(span)[:2 * (g % 8) + 1]] = False
    w, b = _layer(rng, K, n_out=32)
    act = _activations(rng, K, dead)
    got, steps = Q.grouped_chain(w, b, act, group)
    assert _same_bits(got, Q.dense_chain(w, b, act))
    live = (~dead).sum(axis=1)
    assert np.array_equal(steps, (live + 1) // 2)
    if group == 1:                                         # the shipped kernel: the model of tests/dec_sparse_model.py
        got1, steps1, _ = M.compact_chain(w, b, act)
        assert _same_bits(got1, got) and np.array_equal(steps1, steps)


def test_the_bench_tools_threshold_is_the_kernels():
    """tools/bench_kernels.py counts the decoder's executed work with the kernel's own rule for the compacted body"""
    import os
    import re
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import bench_kernels
    from _common import dec_min_dead
    assert bench_kernels.DEC_MIN_DEAD == dec_min_dead()
    hdr = open(os.path.join(root, "3dal_pytorch_amd", "csrc", "dal3_kernels.h")).read()
    assert bench_kernels.BLOB_TAIL_BYTES == 4 * int(re.search(r"^#define DAL3_BLOB_TAIL_FLOATS (\d+)", hdr, re.M).group(1))
