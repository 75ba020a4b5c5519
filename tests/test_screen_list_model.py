"""The list building of the screened max-pools (csrc/dal3_screen.h) on the CPU model tests/screen_list_model.py: every
set hit bit becomes exactly one list entry with the right (channel, point), counts are exact around the round size and
the cap, and a tile over the cap is reported with nothing written."""
import numpy as np
import pytest

import screen_list_model as M

SCR_CAP = 1024                                             # csrc/dal3_enc_screen.hip, csrc/dal3_head_screen.hip (HEAD_SCR_CAP)
SHAPES = [(2, 32), (1, 16)]                                # (tiles per wave, blocks): the encoder's conv5, the heads' conv4


def _pairs(entries):
    return [(int(e) >> 8, int(e) & 31) for e in entries]


def _check(hits, T, cap=SCR_CAP):
    counts, overflow, lists = M.build_lists(M.hit_words(hits), T, cap)
    want = [M.expected_pairs(hits, j) for j in range(T)]
    assert counts == [len(w) for w in want]
    assert overflow == any(c > cap for c in counts)
    if overflow:
        assert all(len(lst) == 0 for lst in lists)
        return counts, overflow
    for j in range(T):
        got = _pairs(lists[j])
        assert len(got) == len(set(got)) == counts[j], "an entry twice"
        assert set(got) == want[j]
        assert all(0 <= c < 32 * hits.shape[0] and 0 <= p < 32 for c, p in got)
    return counts, overflow


def _scattered(rng, nblk, T, j, count):
    """exactly `count` hits in tile j, scattered over blocks, lanes and registers"""
    hits = np.zeros((nblk, 64, T, 16), bool)
    flat = rng.permutation(nblk * 64 * 16)[:count]
    mt, lane, r = np.unravel_index(flat, (nblk, 64, 16))
    hits[mt, lane, j, r] = True
    return hits


def test_bit_order_of_a_hit_word():
    """push s = r T + j ends at bit 16 T - 1 - s: the last register of the last tile is bit 0"""
    for T in (1, 2):
        for r in range(16):
            for j in range(T):
                hits = np.zeros((1, 64, T, 16), bool)
                hits[0, 5, j, r] = True
                w = M.hit_words(hits)
                assert int(w[0, 5]) == 1 << (16 * T - 1 - (r * T + j)) and int(w.sum()) == int(w[0, 5])
                assert int(w[0, 5]) & M.tile_mask(T, j) and not any(int(w[0, 5]) & M.tile_mask(T, k) for k in range(T) if k != j)


@pytest.mark.parametrize("T,nblk", SHAPES)
@pytest.mark.parametrize("density", [0.002, 0.01, 0.03])
def test_random_hits_are_listed_once_each(T, nblk, density):
    rng = np.random.default_rng(int(density * 1e4) + T)
    hits = rng.random((nblk, 64, T, 16)) < density
    counts, overflow = _check(hits, T)
    assert not overflow and all(c > 0 for c in counts)


@pytest.mark.parametrize("T,nblk", SHAPES)
@pytest.mark.parametrize("count", [0, 63, 64, 65, SCR_CAP, SCR_CAP + 1])
def test_counts_around_a_round_and_the_cap(T, nblk, count):
    rng = np.random.default_rng(count)
    for j in range(T):
        hits = _scattered(rng, nblk, T, j, count)
        if T == 2:                                         # the other tile has a list of its own
            hits |= _scattered(rng, nblk, T, 1 - j, 70)
        counts, overflow = _check(hits, T)
        assert counts[j] == count and overflow == (count == SCR_CAP + 1)


@pytest.mark.parametrize("T,nblk", SHAPES)
@pytest.mark.parametrize("per_lane", [1, 2, 3, 16])
def test_several_hits_of_one_lane_in_one_block(T, nblk, per_lane):
    rng = np.random.default_rng(per_lane)
    for j in range(T):
        hits = _scattered(rng, nblk, T, j, 40)
        regs = rng.permutation(16)[:per_lane]
        hits[3, 37, j, regs] = True
        hits[nblk - 2, 0, j, regs] = True
        _check(hits, T)


@pytest.mark.parametrize("T,nblk", SHAPES)
def test_every_lane_hits_in_one_block(T, nblk):
    hits = np.zeros((nblk, 64, T, 16), bool)
    hits[7, :, :, 9] = True
    hits[7, ::2, T - 1, 0] = True
    counts, _ = _check(hits, T)
    assert counts[T - 1] == 96


@pytest.mark.parametrize("T,nblk", SHAPES)
def test_hits_in_the_last_block_only(T, nblk):
    """the last block's epilogue has no MFMAs to ride behind: a code path of its own in the kernels"""
    rng = np.random.default_rng(3)
    hits = np.zeros((nblk, 64, T, 16), bool)
    hits[nblk - 1] = rng.random((64, T, 16)) < 0.05
    counts, overflow = _check(hits, T)
    assert not overflow and all(c > 0 for c in counts)
    hits[:] = False
    hits[nblk - 1, 63, T - 1, 15] = True
    assert _check(hits, T)[0][T - 1] == 1


def test_a_full_tile_overflows_and_writes_nothing():
    """a constant crop: every (channel, point) pair a candidate"""
    hits = np.ones((32, 64, 2, 16), bool)
    counts, overflow = _check(hits, 2)
    assert counts == [32 * 1024, 32 * 1024] and overflow
