"""dconv2's grouped consumer on the CPU (tests/dec_group_model.py): the kernel's rows, list, leftover row and pad give the
accumulators of `grouped_chain` bit for bit, and after the ReLU the dense chain's. K = 512, 256 outputs, 64 points (two
tiles, the second with the live set mirrored so that both ends of the chain are exercised), group sizes 1, 2, 4 and 8;
the live sets are those of tests/test_gpu_dec_group.py."""
import numpy as np
import pytest

import dec_group_model as G
import dec_queue_model as Q

K, N_OUT, POINTS = 512, 256, 64


def _case(group, live, seed):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((N_OUT, K)).astype(np.float32)
    b = rng.standard_normal(N_OUT).astype(np.float32)
    dead = np.stack([~live, ~live[::-1]])                  # tile 1: the mirrored set
    a = np.maximum(rng.standard_normal((K, POINTS)), 0).astype(np.float32)
    a[:, ::Q.TILE] = np.float32(0.5)
    act = np.zeros_like(a)
    act[Q.chain(K)] = a[Q.chain(K)] * np.repeat(~dead.T, Q.TILE, axis=1)
    assert np.array_equal(Q.live_rows(act), ~dead)
    return w, b, act, (~dead).sum(axis=1)


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("group", [1, 2, 4, 8])
def test_the_kernels_rows_list_and_leftover_give_the_grouped_chain(group):
    for seed, (name, live) in enumerate(G.live_sets(group).items()):
        w, b, act, n_live = _case(group, live, seed)
        got, steps = G.kernel_chain(w, b, act, group)
        want, want_steps = Q.grouped_chain(w, b, act, group)
        assert _same_bits(got, want), name
        assert np.array_equal(steps, want_steps) and np.array_equal(steps, (n_live + 1) // 2), name
        dense = Q.dense_chain(w, b, act)
        assert _same_bits(np.maximum(got, 0) + np.float32(0), np.maximum(dense, 0) + np.float32(0)), name


@pytest.mark.parametrize("group", [1, 2, 4, 8])
@pytest.mark.parametrize("n_flight", [3, 4])
def test_the_read_ahead_stays_inside_the_list_at_every_depth(group, n_flight):
    """a full group behind a leftover is the longest list there is: 1 + 32 group entries and the entries read ahead"""
    live = np.zeros(K, bool)
    live[0] = True
    live[K - 32 * group:] = True
    w, b, act, _ = _case(group, live, 7)
    got, _ = G.kernel_chain(w[:8], b[:8], act, group, n_flight=n_flight)
    assert _same_bits(got, Q.grouped_chain(w[:8], b[:8], act, group)[0])


def test_a_leftover_read_from_its_old_row_would_be_wrong():
    """the model's rows are overwritten by every group as in LDS: without the copy to PEND_ROW the bits change"""
    group = 4
    live = G.live_sets(group)["leftover across dead groups"]
    w, b, act, _ = _case(group, live, 1)
    keep = G.PEND_ROW
    try:
        G.PEND_ROW = 3                                     # "leave it where it was": the next group's dead row 3 lands on it
        bad, _ = G.kernel_chain(w, b, act, group)
    finally:
        G.PEND_ROW = keep
    assert not _same_bits(bad, Q.grouped_chain(w, b, act, group)[0])


def test_the_models_constants_are_the_kernels():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "3dal_pytorch_amd", "csrc", "dal3_pointmlp.hip")).read()
    assert int(re.search(r"^#define DEC_Q_ZERO (\d+)", src, re.M).group(1)) == Q.ZERO_ROW
    assert int(re.search(r"^#define DEC_Q_OVER (\d+)", src, re.M).group(1)) == Q.LIST_OVER
    assert "#define DEC_G_PEND ((DEC_Q_ZERO + 1) + DEC_Q_LIST / 32)" in src and G.PEND_ROW == 266
    assert int(re.search(r"^#define DAL3_DEC_GROUP (\d+)", src, re.M).group(1)) in (1, 2, 4, 8)
