"""The fp32 decoder's pair of waves on the CPU (tests/dec_pair_model.py): with the model's rows, buffers, mask exchange, lists,
leftover rule and barriers, every accumulator of dconv2 - dconv4 and every logit has the bits of the one-wave chains
(`dec_queue_model.grouped_chain`, `queue_chain`), no row is read before it is written, and none is overwritten before its
last reader has passed a barrier — in both orders of the two waves. The live sets are those of tests/dec_group_model.py,
the plans are `dec_prune_model.plan`'s. The judge rejects the planted faults."""
import numpy as np
import pytest

import dec_group_model as G
import dec_pair_model as M
import dec_prune_model as P
import dec_queue_model as Q

IDENT = np.arange(P.PLAN_LD).clip(max=P.NULL_K)            # InsSegW::dec_ident: chain index = list position


def _act(live, rng):
    """live bool (n,) by list position -> relu(dconv1) of one tile, (n, TILE): a dead row is +0 in every point, a live row
    has zeros among its points and one point that is surely not zero"""
    a = np.maximum(rng.standard_normal((len(live), Q.TILE)), 0).astype(np.float32)
    a[:, 0] = np.float32(0.5)
    return a * live[:, None]


def _odd(live, rng):
    """the same set with an odd count (odd totals in dconv3 / dconv4)"""
    live = live.copy()
    if live.sum() % 2 == 0:
        live[rng.integers(len(live))] ^= True
    return live


def _consecutive_odd():
    """1, 2, 4 and 1 live rows in the four groups: the totals are 1, 3, 5 and 2, so a leftover is written in three
    consecutive groups, each while the one before is still entry 0 of the list (`odd per group` alternates: its leftover
    makes every second total even)"""
    live = np.zeros(512, bool)
    live[[5, 128 + 31, 128 + 32, 256, 256 + 63, 256 + 64, 256 + 127, 384 + 77]] = True
    return live


SETS = dict(G.live_sets(M.GROUP))
SETS["odd totals in consecutive groups"] = _consecutive_odd()


@pytest.mark.parametrize("name", list(SETS))
def test_identity_plan_has_the_one_wave_bits_and_no_hazard(name):
    live = SETS[name]
    rng = np.random.default_rng(sorted(SETS).index(name))
    W = M.weights(rng, dead3=~_odd(live[:256], rng), dead4=~_odd(live[-128:], rng))
    out = M.judge(_act(live, rng), IDENT, 16, W)
    assert out["steps2"][0] == (int(live.sum()) + 1) // 2


def test_the_sets_cover_the_seams():
    """what the schedule can get wrong shows only on some sets: say that they are there"""
    span = 32 * M.GROUP
    per_group = lambda live: live.reshape(-1, span).sum(axis=1)
    n = per_group(SETS["odd per group"])
    assert (n % 2 == 1).all()                                                 # a leftover crosses every group seam
    n = per_group(SETS["leftover across dead groups"])
    assert n[0] == 1 and n[-1] == 1 and (n[1:-1] == 0).all()                  # dead groups between two live ones
    assert list(per_group(SETS["odd totals in consecutive groups"])) == [1, 2, 4, 1]
    assert per_group(SETS["nothing live"]).sum() == 0 and SETS["longest list"].reshape(-1, span).all(axis=1).any()


def test_nothing_dead_runs_the_identity_plan_fully_live():
    rng = np.random.default_rng(40)
    live = np.ones(512, bool)
    out = M.judge(_act(live, rng), IDENT, 16, M.weights(rng))
    assert out["steps2"] == [256, 256]


@pytest.mark.parametrize("n_live, nch", [(0, 2), (1, 2), (40, 2), (170, 6), (300, 10), (447, 14)])
def test_plans_and_their_shorter_last_group(n_live, nch):
    """nch = 2: the shortest last group; 6 and 10: a last group of two chunks behind full ones; 14: the second buffer last"""
    rng = np.random.default_rng(50 + n_live)
    flagged = np.ones(512, bool)
    flagged[rng.permutation(512)[:n_live]] = False
    gb = rng.standard_normal(512).astype(np.float32)
    pk, gbc, got_nch = P.plan(flagged, gb)
    P.judge_plan(pk, gbc, got_nch, flagged, gb)
    assert got_nch == nch
    live = np.zeros(32 * nch, bool)                        # the plan's channels, a fifth of them dead in this tile; the padding is dead
    live[:n_live] = rng.random(n_live) >= 0.2
    W = M.weights(rng, dead3=rng.random(256) < 0.5, dead4=rng.random(128) < 0.5)
    M.judge(_act(live, rng), pk, nch, W)


def _rejects(fault, live, nch=16, pk=IDENT, seed=9):
    rng = np.random.default_rng(seed)
    W = M.weights(rng)
    act = _act(live, rng)
    M.judge(act, pk, nch, W)                               # the schedule itself passes on this input
    with pytest.raises(AssertionError):
        M.judge(act, pk, nch, W, fault=fault)


def test_the_judge_rejects_a_single_buffered_group():
    _rejects("single buffer", SETS["random 0.45"])


def test_the_judge_rejects_a_missing_barrier_before_dconv3s_rows():
    _rejects("no barrier before dconv3", SETS["random 0.45"])


def test_the_judge_rejects_a_leftover_row_owned_by_one_wave():
    _rejects("leftover of one wave", SETS["odd totals in consecutive groups"])


def test_the_judge_rejects_dconv5_summed_as_two_halves():
    _rejects("dconv5 in two halves", SETS["random 0.45"])
    rng = np.random.default_rng(3)                         # and by the bits alone: no hazard is involved
    W = M.weights(rng)
    act = _act(SETS["random 0.45"], rng)
    out, hazards, _ = M.run_tile(act, IDENT, 16, W, fault="dconv5 in two halves")
    assert not hazards
    assert not np.array_equal(out["logits"].view(np.uint32), M.reference_tile(act, IDENT, 16, W)[3].view(np.uint32))


def test_every_planted_fault_has_a_test():
    assert set(M.FAULTS) == {"single buffer", "no barrier before dconv3", "leftover of one wave", "dconv5 in two halves"}


def test_the_models_constants_are_the_kernels():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "3dal_pytorch_amd", "csrc", "dal3_pointmlp.hip")).read()
    assert int(re.search(r"^#define DAL3_DEC_GROUP (\d+)", src, re.M).group(1)) == M.GROUP
    assert M.NULL_K == P.NULL_K and 32 * M.GROUP * 2 == Q.ZERO_ROW   # two buffers of a group's rows fill dconv3's 256
