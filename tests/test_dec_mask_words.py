"""The live mask word of 16 accumulator registers on the CPU (csrc/dal3_pointmlp.hip, note_halves / live_word; DESIGN.md
"Compacted dconv2 - dconv4", mask words): the halves of ballot r in lanes 2 r and 2 r + 1 of one register and one compare of
that register give the word the scalar folding gave — bit 2 r + h = register r, lane half h — and that word is
tests/dec_queue_model.py's live rows in chain order."""
import numpy as np

import dec_queue_model as Q


def _ballots(tile):
    """tile (16, 64) uint32: register r of the 64 lanes -> the 16 wave ballots of `bits != 0`"""
    return [sum(1 << lane for lane in range(64) if tile[r, lane] != 0) for r in range(16)]


def word_scalar(ballots):
    """the folding up to round 14: s_min_u32 half, 1 twice, shift-add, shift, OR"""
    m = 0
    for r, bal in enumerate(ballots):
        lo, hi = min(bal & 0xFFFFFFFF, 1), min(bal >> 32, 1)
        m |= ((hi << 1) + lo) << (2 * r)
    return m


def word_lanes(ballots):
    """note_halves and live_word: v_writelane_b32 of the halves, one v_cmp_ne_u32 of the register, the ballot's low word"""
    halves = [0] * 64                                      # one vector register, lanes 32 .. 63 stay 0
    for r, bal in enumerate(ballots):
        halves[2 * r] = bal & 0xFFFFFFFF
        halves[2 * r + 1] = bal >> 32
    return sum(1 << lane for lane in range(64) if halves[lane] != 0) & 0xFFFFFFFF


def test_lane_form_equals_the_scalar_folding():
    rng = np.random.default_rng(15)
    cases = [np.zeros((16, 64), np.uint32), np.ones((16, 64), np.uint32)]
    for lane in (0, 31, 32, 63):                           # one point of one half, at the halves' edges
        t = np.zeros((16, 64), np.uint32)
        t[5, lane] = 0x7FC00000                            # a NaN's bits are live
        cases.append(t)
    for p in (0.02, 0.5, 0.98):
        cases.append((rng.random((16, 64)) < p).astype(np.uint32) * rng.integers(1, 2**31, (16, 64)).astype(np.uint32))
    for p in (0.3, 0.7):                                   # whole rows dead, as after a ReLU with a negative per-crop term
        t = rng.integers(1, 2**31, (16, 64)).astype(np.uint32)
        t[rng.random(16) < p, :32] = 0
        t[rng.random(16) < p, 32:] = 0
        cases.append(t)
    for t in cases:
        b = _ballots(t)
        assert word_lanes(b) == word_scalar(b)
    assert word_lanes(_ballots(cases[1])) == 0xFFFFFFFF and word_lanes(_ballots(cases[2])) == 1 << 10
    assert word_lanes(_ballots(cases[5])) == 1 << 11


def test_the_word_is_the_queue_models_live_rows_in_chain_order():
    """a 32-channel k-tile of post-ReLU activations in the MFMA accumulator layout: register r holds channel tile_chan(r, 0)
    in lanes 0 .. 31 and tile_chan(r, 1) in lanes 32 .. 63"""
    rng = np.random.default_rng(16)
    act = np.maximum(rng.standard_normal((32, Q.TILE)), 0).astype(np.float32)
    act[rng.random(32) < 0.5] = 0
    act[7, 3] = np.inf
    ch = Q.chain(32)
    regs = np.zeros((16, 64), np.uint32)
    for r in range(16):
        for h in (0, 1):
            regs[r, 32 * h:32 * h + 32] = act[ch[2 * r + h]].view(np.uint32)
    word = word_lanes(_ballots(regs))
    live = Q.live_rows(act)[0]
    assert [(word >> k) & 1 for k in range(32)] == live.astype(int).tolist()
