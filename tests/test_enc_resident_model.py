"""The crop-resident screened encoder (csrc/dal3_enc_screen.hip, ins_seg_encode_resident_kernel) on the CPU.

tests/enc_resident_model.py restates the slot map, round 0's bound phase and the threshold table that rises from
round to round on top of tests/screen_model.py; the crops, weights and `Case` are those of
tests/test_enc_screen_subset_model.py. Every round is held to what the proof promises: the table never exceeds the
final value, a skipped live pair cannot raise the pooled value, the fp32 arg-max is a candidate unless the table holds
the final value already; after the last round the table IS the final value. The candidate counts are printed (-s)."""
import functools
import json

import pytest
import torch

import enc_resident_model as M
import screen_model as S
import test_enc_screen_subset_model as SUB
from _common import synth


def _run(case):
    cand, G0, rep = M.run(case)
    print(json.dumps(rep))
    return cand, G0, rep


def test_slot_map_visits_every_slot_once_and_slot_zero_first():
    for N in (1, 64, 65, 255, 256, 257, 300, 1000, 1024, 1088, 4096, 5120):
        rounds = M.slot_map(N)
        slots = -(-N // 64)
        assert sorted(s for r in rounds for s in r) == list(range(slots)) and rounds[0][0] == 0
        assert len(rounds) == -(-slots // 4) and all(1 <= len(r) <= 4 for r in rounds)
        R = len(rounds)
        assert rounds[0] == [R * w for w in range(4) if R * w < slots]


def test_bench_crops_need_fewer_candidates_than_the_two_launches():
    """the 32 bench crops: round 0's table is pass A's at the shipped stride of 4 (slots 0, 4, 8, 12), so no tile can
    exceed the list where the two launches' do not; the mean per 32-point tile falls (model: 217.0 -> 130.7)"""
    case = SUB._bench()
    cand, G0, rep = _run(case)
    two, G_two = SUB.subset_rule(case.s16, case.E, case.b5, case.dense, 4)
    assert torch.equal(G0.float(), G_two)
    c32 = two.view(32, 1024, -1, 32).sum((1, 3))
    two_mean, two_max = float(c32.double().mean()), int(c32.max())
    print(json.dumps({"two_launch_per_tile_mean": two_mean, "two_launch_per_tile_max": two_max}))
    assert bool((two | ~cand).all()), "a resident candidate that the two launches do not have"
    assert rep["per_tile_mean"] < two_mean
    assert rep["per_tile_max"] <= S.SCR_CAP and rep["tiles_over_cap"] == 0.0
    assert rep["per_round"] == sorted(rep["per_round"], reverse=True)


@pytest.mark.parametrize("scale5,shift5", [(1.0, 0.0), (1e3, 0.0), (1e-3, 0.0), (1.0, -50.0)])
def test_adversarial_crops(scale5, shift5):
    """ties, constant crops, huge and tiny coordinates, a useless bound, dense waves inside and outside round 0; conv5
    scaled by 1e3 / 1e-3, channels whose maximum is negative"""
    _run(SUB._adv(scale5, shift5))


@pytest.mark.parametrize("N", [64, 65, 300, 1000])
def test_short_and_ragged_crops(N):
    """one slot, two slots (idle waves in the only round), a last round that is not full"""
    _run(SUB.Case(synth.state_dict("static_one", seed=7), synth.static_crops(6, N, seed=N)[0], f"ragged {N}"))


def test_long_crops():
    """N = 5120: 80 slots, 20 rounds (model: 75.5 -> 46.5 candidates per tile)"""
    case = SUB.Case(synth.state_dict("static_one", seed=7), synth.static_crops(6, 5120, seed=5120)[0], "N = 5120")
    cand, _, rep = _run(case)
    two, _ = SUB.subset_rule(case.s16, case.E, case.b5, case.dense, 4)
    assert int(cand.sum()) < int(two.sum()) and rep["tiles_over_cap"] == 0.0


@functools.lru_cache(maxsize=None)
def _small():
    return SUB.Case(synth.state_dict("static_one", seed=7), synth.static_crops(6, 1000, seed=1000)[0], "judge")


def test_judge_accepts_the_model_and_the_contiguous_map():
    assert M.judge(_small()) is None
    assert M.judge(_small(), slot_map=M.contiguous_slot_map) is None


def test_judge_rejects_a_bound_phase_without_the_error_term():
    forgot = lambda m, Ew, b: m + b
    why = M.judge(_small(), bound_phase=forgot)
    assert why is not None and "above the dense result" in why


def test_judge_rejects_a_slot_map_that_skips_a_slot():
    def skips(N):
        rounds = M.slot_map(N)
        return rounds[:-1] + [rounds[-1][:-1]]
    why = M.judge(_small(), slot_map=skips)
    assert why is not None and ("never visited" in why or "not the dense result" in why)
