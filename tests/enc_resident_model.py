"""tests/enc_resident_model.py — a CPU MODEL of the crop-resident screened encoder (csrc/dal3_enc_screen.hip,
ins_seg_encode_resident_kernel; test infrastructure on top of tests/screen_model.py, which is imported unchanged).

One workgroup of four waves owns a crop. A slot is 64 consecutive points; with slots = ceil(N / 64) and
R = ceil(slots / 4) the kernel runs R rounds and wave w takes slot r + R w in round r. Round 0 starts with the bound
phase — pass A's sweep on the round's own slots: G0 = relu(fl(max s16 - E + b)) — and every round screens its points
against the threshold table as it stands, which later rounds find raised by the exact values of the rounds before.
The proof of the screen needs "G <= the final value" and nothing else, so any such table keeps the dense bits.

The model is PESSIMISTIC in the way the kernel cannot be: the table is held constant within a round and raised after
it by the exact relu(chain + b) maxima of that round's points (on the device a wave also sees what the other waves of
its own round have added by the time it reads). float64 on the fp32 operands stands in for the chain, as in
screen_model."""
import numpy as np
import torch

import screen_model as S

WAVES = 4                                                  # DAL3_WG_WAVES


def slot_map(N):
    """-> list over the rounds of the slots (of 64 points) that the four waves take; every slot exactly once"""
    slots = -(-N // S.WAVE_POINTS)
    R = -(-slots // WAVES)
    return [[r + R * w for w in range(WAVES) if r + R * w < slots] for r in range(R)]


def contiguous_slot_map(N):
    """the variant of the issue's item 5: round r takes slots 4 r .. 4 r + 3"""
    slots = -(-N // S.WAVE_POINTS)
    return [list(range(r, min(r + WAVES, slots))) for r in range(0, slots, WAVES)]


def bound_phase(m, Ew, b):
    """pass A's epilogue on the visited waves: m = max_p s16 per (crop, channel, wave), Ew the waves' bounds, all fp32 ->
    the contribution to G before the ReLU, (B, 1024, waves)"""
    return (m - (m.abs() * torch.tensor(2.0 ** -22, dtype=torch.float32) + Ew)) + b


def run(case, slot_map=slot_map, bound_phase=bound_phase):
    """case: test_enc_screen_subset_model.Case. Runs the rounds, asserts per round what the proof promises and at the end
    that the table IS the final value; returns (candidates (B,1024,N) bool, report)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    N, s16, E, dense, live, exact = case.N, case.s16, case.E, case.dense, case.live, case.exact
    B = s16.shape[0]
    b32 = case.b5.float()[None, :, None]
    b64 = case.b5.double()[None, :, None]
    final = torch.relu(exact.amax(2) + b64[:, :, 0])                               # (B,1024) float64; dense waves left out
    has_live = live.any(2)
    arg = exact.argmax(2)                                                          # (B,1024)
    rounds = slot_map(N)
    slot_of = torch.arange(N) // S.WAVE_POINTS

    # round 0's bound phase (a visited wave that leaves the screen contributes nothing)
    m = S._waves(torch.where(live, s16, torch.full_like(s16, -np.inf)), N).amax(-1)            # (B,1024,waves)
    Ew = S._waves(E, N)[..., 0]
    first = torch.tensor(rounds[0])
    G = torch.relu(bound_phase(m[..., first], Ew[..., first], b32).amax(2)).double()            # -inf + b = -inf -> 0
    G0 = G.clone()

    cand = torch.zeros_like(live)
    seen = torch.zeros(N, dtype=torch.bool)
    per_round = []
    for r, slots in enumerate(rounds):
        pts = torch.isin(slot_of, torch.tensor(slots))
        assert not bool((pts & seen).any()), (case.what, r, "a slot is visited twice")
        seen |= pts
        assert bool((G <= final).all()), (case.what, r, "the threshold table is above the dense result")
        G32 = G.float()[:, :, None]                        # (the 2^-22 term of thr covers this rounding)
        thr = (G32 - b32) - ((G32.abs() + b32.abs()) * f(2.0 ** -22) + E[:, :, pts])
        c = (s16[:, :, pts] > thr) & live[:, :, pts]
        ex = exact[:, :, pts]
        skipped = ~c & live[:, :, pts]
        assert bool(((ex + b64)[skipped] <= G[:, :, None].expand_as(ex)[skipped]).all()), (case.what, r, "a skipped pair could raise g")
        here = pts[arg]                                    # (B,1024): the crop's fp32 arg-max lies in this round
        at = cand.new_zeros(B, 1024, N)
        at[:, :, pts] = c
        ok = at.gather(2, arg[:, :, None])[:, :, 0] | (G >= final) | ~has_live | ~here
        assert bool(ok.all()), (case.what, r, "the fp32 arg-max is not a candidate and G is below the final value")
        cand |= at
        per_round.append(float(c.sum()) / max(1, B * -(-int(pts.sum()) // 32)))
        # the round's exact values: candidates only — a skipped pair cannot raise the table (asserted above)
        G = torch.maximum(G, torch.relu(torch.where(c, ex + b64, torch.full_like(ex, -np.inf)).amax(2)))
    assert bool(seen.all()), (case.what, "a slot is never visited")
    assert bool((G == final)[has_live].all()), (case.what, "the crop's table is not the dense result after the last round")
    c32 = torch.nn.functional.pad(cand, (0, (-N) % 32)).view(B, 1024, -1, 32).sum((1, 3))
    rep = {"what": case.what, "rounds": len(rounds), "per_tile_mean": float(c32.double().mean()), "per_tile_max": int(c32.max()),
           "tiles_over_cap": float((c32 > S.SCR_CAP).double().mean()), "per_round": [round(v, 1) for v in per_round]}
    return cand, G0, rep


def judge(case, slot_map=slot_map, bound_phase=bound_phase):
    """-> None if the variant keeps every promise on `case`, else the reason it was rejected"""
    try:
        run(case, slot_map, bound_phase)
    except AssertionError as e:
        return str(e.args[0] if e.args else e)
    return None
