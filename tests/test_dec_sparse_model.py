"""The compaction order of the fp32 decoder's dconv2 on the CPU (tests/dec_sparse_model.py): dropping the channels that
are dead in a whole 32-point tile, pairing the live ones two by two with a carry across chunks and a final zero pad,
gives the dense fmaf chain's bits; and the dead fractions the change was sized from still hold on the bench crops."""
import numpy as np
import pytest
import torch

import dec_sparse_model as M
from _common import synth
from oracle import ref_heads as R


def _weights(rng, n_out=64):
    return rng.standard_normal((n_out, 512)).astype(np.float32), rng.standard_normal(n_out).astype(np.float32)


def _activations(rng, n_tiles, dead):
    """post-ReLU activations (512, 32 n_tiles): ~half of the elements +0, and per tile the chain positions in `dead`
    (bool (n_tiles, 512)) +0 in all 32 points"""
    a = np.maximum(rng.standard_normal((512, n_tiles * M.TILE)), 0).astype(np.float32)
    a[:, ::M.TILE] = np.float32(0.5)                       # every channel is live somewhere in its tile ...
    keep = np.repeat(~dead.T, M.TILE, axis=1)              # ... unless the case kills it there
    out = np.zeros_like(a)
    out[M.CHAIN] = a[M.CHAIN] * keep
    return out


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _run(rng, dead, what):
    w2, b2 = _weights(rng)
    act = _activations(rng, dead.shape[0], dead)
    assert np.array_equal(M.live_masks(act), ~dead), what
    want = M.dense_chain(w2, b2, act)
    got, steps, dense = M.compact_chain(w2, b2, act)
    assert _same_bits(got, want), what
    return steps, dense, (~dead).sum(axis=1)


@pytest.mark.parametrize("p_dead", [0.1, 0.46, 0.9])
def test_random_dead_channels_reproduce_the_dense_chain(p_dead):
    rng = np.random.default_rng(int(p_dead * 100))
    dead = rng.random((6, 512)) < p_dead
    steps, dense, live = _run(rng, dead, f"random {p_dead}")
    assert np.array_equal(steps, (live + 1) // 2)


def test_carry_across_chunks_and_the_final_pad():
    """odd live counts in every chunk (the carry alternates), a lone live channel whose partner arrives eight chunks
    later, a lone channel that is never paired (the zero pad), nothing live at all, nothing dead at all"""
    rng = np.random.default_rng(5)
    dead = np.ones((6, 512), bool)
    for c in range(16):                                    # tile 0: 2 c + 1 live channels in chunk c
        dead[0, 32 * c + rng.permutation(32)[:2 * c + 1]] = False
    dead[1, 32 * 2 + 7] = dead[1, 32 * 10 + 30] = False    # tile 1: one carry over empty chunks
    dead[1, 32 * 11:32 * 12] = False                       # ... followed by a full chunk with nothing pending
    dead[2, 32 * 15 + 31] = False                          # tile 2: only the last channel of all (padded)
    dead[3, 0] = False                                     # tile 3: only the first (carried to the end, padded)
    dead[5] = False                                        # tile 4: all dead; tile 5: all live
    steps, dense, live = _run(rng, dead, "carry")
    assert steps.tolist() == [128, 17, 1, 1, 0, 256]
    assert dense.tolist() == [0, 1, 0, 0, 0, 16]


def test_a_full_chunk_behind_a_pending_channel_is_not_dense():
    rng = np.random.default_rng(6)
    dead = np.ones((1, 512), bool)
    dead[0, 5] = False
    dead[0, 32:64] = False
    steps, dense, _ = _run(rng, dead, "pending + full")
    assert steps.tolist() == [17] and dense.tolist() == [0]


def test_bench_crops_keep_the_dead_fractions_the_change_was_sized_from():
    """the first 32 bench crops (synth.static_crops / synth.state_dict("static_one"), as bench.py builds them), BN folded,
    fp32 torch: fraction of zero elements, of (32-point tile, channel) pairs that are all zero, of channels zero over the
    whole crop, for the inputs of dconv2 / dconv3 / dconv4. The figures are the design table's; weights and crops are
    deterministic, so they hold to the printed digits (0.0005) plus the elements whose pre-activation the CPU matmul's
    summation order can move across zero (a few in 10^5): 0.002."""
    pts = torch.from_numpy(synth.static_crops(32, 1024)[0]).transpose(2, 1)
    xs = M.decoder_inputs(R.as_torch_sd(synth.state_dict("static_one")), pts)
    table = [(0.509, 0.459, 0.438), (0.480, 0.446, 0.436), (0.433, 0.386, 0.379)]
    for x, want, name in zip(xs, table, ("dconv2", "dconv3", "dconv4")):
        got = M.dead_fractions(x)
        print(name, "input: elements = 0 %.4f, (tile, channel) all zero %.4f, channel zero over the crop %.4f" % got)
        assert all(abs(g - w) < 0.002 for g, w in zip(got, want)), (name, got, want)
    # what the kernel runs on these crops: ceil(live / 2) compact k-steps per tile against 256 dense ones
    act = xs[0][0].numpy()
    live = M.live_masks(np.ascontiguousarray(act)).sum(axis=1)
    print("crop 0: live channels per tile %.1f of 512, compact k-steps %.1f of 256" % (live.mean(), ((live + 1) // 2).mean()))
