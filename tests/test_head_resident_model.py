"""The item-resident screened point head (csrc/dal3_head_screen.hip, point_head_resident_kernel) on the CPU.

tests/head_resident_model.py restates the slot map, round 0's bound phase and the threshold table that rises from round
to round on top of tests/head_screen_model.py. Every round is held to what the proof promises: the table never exceeds
the final value, a skipped real pair cannot raise the pooled value, the fp32 arg-max is a candidate (or a point of a dense
tile) unless the table holds the final value already; after the last round the table IS the final value. The candidate
counts are printed (-s)."""
import functools
import json

import numpy as np
import pytest
import torch

import head_resident_model as M
import head_screen_model as H
from _common import synth


def _run(case):
    cand, G0, rep = M.run(case)
    print(json.dumps(rep))
    return cand, G0, rep


@functools.lru_cache(maxsize=None)
def _bench():
    sd = synth.state_dict("static_one")
    obj, distinct = H.bench_objects(32, sd)
    return sd, obj, distinct


def test_slot_map_visits_every_tile_once_and_tile_zero_first():
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 80):
        rounds = M.slot_map(n)
        assert sorted(t for r in rounds for t in r) == list(range(n)) and rounds[0][0] == 0
        assert len(rounds) == -(-n // 4) and all(1 <= len(r) <= 4 for r in rounds)
        R = len(rounds)
        assert rounds[0] == [R * w for w in range(4) if R * w < n]
        flat = M.contiguous_slot_map(n)
        assert sorted(t for r in flat for t in r) == list(range(n)) and len(flat) == R


def test_bench_objects_need_fewer_candidates_than_the_two_launches():
    """the first 32 bench crops' object points (11.4 live tiles per item): every live tile is screened, the mean per tile lies
    below the two launches' mean per SCREENED tile at the shipped stride of 4 (which computes a quarter of the live tiles
    densely on top), no tile exceeds the list, no tile leaves the screen, and the per-round means fall"""
    sd, obj, distinct = _bench()
    case = M.Case(sd, obj, distinct, what="bench")
    _, _, rep = _run(case)
    two = H.run(sd, obj, distinct, stride=4, what="bench, two launches")
    print(json.dumps(two))
    assert rep["live_tiles"] == two["live_tiles"]
    assert rep["per_tile_mean"] < two["cand_mean"]
    assert rep["per_tile_max"] <= H.SCR_CAP and rep["tiles_over_cap"] == 0 and rep["tiles_dense_for_range"] == 0
    assert rep["per_round"] == sorted(rep["per_round"], reverse=True)
    assert sum(rep["tiles_per_round"]) == rep["live_tiles"]
    assert 0.0 <= rep["idle_wave_rounds"] < 0.10


@pytest.mark.parametrize("scale4,shift4", [(1.0, 0.0), (1e3, 0.0), (1e-3, 0.0), (1.0, -50.0)])
def test_adversarial_items(scale4, shift4):
    """head_screen_model.adversarial — duplicated points (exact ties), all points equal (the list overflows: dense tiles),
    one live point, coordinates x 1e4 (dense for range, in round 0 and later: no bound from them) and x 1e-6 — with conv4
    scaled by 1e3 / 1e-3 and a bias shift that makes half of the channel maxima negative (pooled value +0)"""
    _, obj, distinct = _bench()
    o, d = H.adversarial(obj[:8], distinct[:8])
    sd = synth.state_dict("static_one", seed=91)
    case = M.Case(sd, o, d, what=f"adversarial x{scale4:g} {shift4:+g}", scale4=scale4, shift4=shift4)
    _, G0, rep = _run(case)
    assert rep["tiles_dense_for_range"] == 16                                  # item 3, every tile
    if scale4 == 1.0 and shift4 == 0.0:
        assert rep["tiles_over_cap"] >= 4                                      # item 1: round 0's tiles at the least
    if shift4:
        assert float((G0[:, ::2] == 0).float().mean()) > 0.9


@pytest.mark.parametrize("tiles", [1, 2, 4, 5, 15, 16])
def test_short_and_ragged_items(tiles):
    """items of 1, 2, 4, 5, 15 and 16 live tiles, the last tile whole, holding one point, and holding 31: idle waves at round
    0's barrier, a second round of one wave, a last round that is not full"""
    _, obj, _ = _bench()
    d = np.array([32 * tiles, 32 * (tiles - 1) + 1, 32 * tiles - 1, 32 * (tiles - 1) + 17], np.int32)
    case = M.Case(synth.state_dict("static_one", seed=7), obj[8:12], d, what=f"{tiles} live tiles")
    _, _, rep = _run(case)
    assert rep["live_tiles"] == 4 * tiles and rep["rounds"] == -(-tiles // 4)


def test_point_emb_at_2560_points():
    """head kind 2, M = 2560: 80 tiles, 20 rounds. Round 0 bounds the table from 4 of up to 80 tiles where the two launches'
    seeds are a quarter of them, so the mean per tile is NOT below the two launches' here (model: 51.5 per live tile, all 223
    screened, against 48.0 per screened tile with 57 of the 223 dense as seeds); what is held is the proof and the list"""
    sd = synth.state_dict("dynamic", seed=23)
    x = np.ascontiguousarray(synth.dynamic_items(4, seed=5)[0][:, :2560, :4]).astype(np.float32)
    assert x.shape == (4, 2560, 4)
    d = np.array([2560, 2559, 1281, 700], np.int32)
    for b in range(4):
        x[b, d[b]:] = x[b, np.arange(2560 - d[b]) % d[b]]
    case = M.Case(sd, x, d, p="point_emb", what="point_emb 4 x 2560")
    _, _, rep = _run(case)
    two = H.run(sd, x, d, p="point_emb", stride=4, what="point_emb, two launches")
    print(json.dumps(two))
    assert rep["rounds"] == 20 and rep["tiles_over_cap"] == 0 and rep["per_tile_max"] <= H.SCR_CAP
    assert rep["live_tiles"] == two["live_tiles"] and rep["per_round"][0] == max(rep["per_round"])


@functools.lru_cache(maxsize=None)
def _small():
    _, obj, distinct = _bench()
    return M.Case(synth.state_dict("static_one", seed=7), obj[:6], distinct[:6], what="judge")


def test_judge_accepts_the_model_and_the_contiguous_map():
    assert M.judge(_small()) is None
    assert M.judge(_small(), slot_map=M.contiguous_slot_map) is None


def test_judge_rejects_a_bound_phase_without_the_error_term():
    forgot = lambda m, E, b: m + b
    why = M.judge(_small(), bound_phase=forgot)
    assert why is not None and "above the dense result" in why


def test_judge_rejects_a_slot_map_that_skips_a_tile():
    def skips(n):
        rounds = M.slot_map(n)
        return rounds[:-1] + ([rounds[-1][:-1]] if len(rounds[-1]) > 1 else [])
    why = M.judge(_small(), slot_map=skips)
    assert why is not None and "never visited" in why
