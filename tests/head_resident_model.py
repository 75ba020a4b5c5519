"""tests/head_resident_model.py — a CPU MODEL of the item-resident screened point head (csrc/dal3_head_screen.hip,
point_head_resident_kernel; test infrastructure on top of tests/head_screen_model.py, which is imported unchanged).

One workgroup of four waves owns an item. A tile is 32 consecutive points; with n = the item's live tiles and
R = ceil(n / 4) the kernel runs R rounds and wave w takes tile r + R w in round r. Round 0 starts with the bound phase on
the round's own tiles — G0 = relu(fl(fl(m - fl(|m| 2^-22 + E)) + b)), m the tile's maximum fp16 score over its real
points — and every round screens its tiles against the threshold table as it stands, which later rounds find raised by
the exact values of the rounds before. NO tile is dense for being a seed. The proof of the screen needs "G <= the final
value" and nothing else, so any such table keeps the dense bits.

The model is PESSIMISTIC in the way the kernel cannot be: the table is held constant within a round and raised after it
by the exact relu(chain + b) maxima of that round's tiles (on the device a wave also sees what the other waves of its own
round have added by the time it reads). A tile that leaves the screen — activations beyond fp16's range, or more
candidates than the list holds — is computed densely: it gives no bound, and all its exact values reach the table.
float64 on the fp32 operands stands in for the chain, as in head_screen_model."""
import numpy as np
import torch

import head_screen_model as H
from oracle import ref_heads as R_

WAVES = 4                                                  # DAL3_WG_WAVES
TILE = H.TILE


def slot_map(n):
    """n live tiles -> list over the rounds of the tiles that the four waves take; every tile exactly once"""
    R = -(-n // WAVES)
    return [[r + R * w for w in range(WAVES) if r + R * w < n] for r in range(R)]


def contiguous_slot_map(n):
    """the variant of the issue's item 5: round r takes tiles 4 r .. 4 r + 3"""
    return [list(range(r, min(r + WAVES, n))) for r in range(0, n, WAVES)]


def bound_phase(m, E, b):
    """round 0's epilogue: m = max_p s16 per (item, channel, tile), E the tiles' bounds, b the bias, all fp32 -> the
    contribution to G before the ReLU"""
    return (m - (m.abs() * torch.tensor(2.0 ** -22, dtype=torch.float32) + E)) + b


class Case:
    """one batch through conv1..conv3 and both evaluations of conv4: x (B,M,C) fp32 points, distinct (B,) or None"""

    def __init__(self, sd, x, distinct, p="box_est", what="", scale4=1.0, shift4=0.0):
        f = lambda v: torch.tensor(v, dtype=torch.float32)
        self.what = what
        sd = R_.as_torch_sd(sd) if not torch.is_tensor(next(iter(sd.values()))) else sd
        xe, live, real = H.effective_points(torch.as_tensor(x).float(), distinct)
        x3, w4, b4 = H.activations(sd, xe.transpose(2, 1), p)
        w4 = (w4 * f(scale4)).float()
        b4 = b4.float().clone()
        b4[::2] += f(shift4)
        B, _, Mp = x3.shape
        nt = Mp // TILE
        self.B, self.Mp, self.nt, self.b4 = B, Mp, nt, b4
        self.live, self.real = live, real                  # (B,nt), (B,Mp)
        self.n_live = live.sum(1)
        x3 = x3.float()
        self.s16 = torch.einsum("oc,bcn->bon", w4.half().float(), x3.half().float())
        self.exact = torch.einsum("oc,bcn->bon", w4.double(), x3.double())
        ss = (x3 * x3).sum(1).view(B, nt, TILE).amax(-1)
        X = torch.sqrt(ss) * f(1.0 + 2.0 ** -15)
        self.range_dense = (x3.amax(1).view(B, nt, TILE).amax(-1) > H.F16_GUARD) & live
        P, Q = (t.float() for t in H.coefficients(w4))
        E = X[:, None, :] * P[None, :, None] + Q[None, :, None]                      # (B,512,nt)
        self.E = E * f(2.0 ** -20) + E
        # the weights themselves beyond fp16 (the blob's flag): every tile is dense
        if not bool(torch.isfinite(w4.half().float()).all()):
            self.range_dense = live.clone()


def _per_pt(t):
    return t.unsqueeze(-1).expand(*t.shape, TILE).reshape(*t.shape[:-1], t.shape[-1] * TILE)


def run(case, slot_map=slot_map, bound_phase=bound_phase):
    """Runs the rounds, asserts per round what the proof promises and at the end that the table IS the final value;
    returns (candidates (B,512,Mp) bool, G0 (B,512), report)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    B, Mp, nt = case.B, case.Mp, case.nt
    s16, exact, E, live, real = case.s16, case.exact, case.E, case.live, case.real
    b32 = case.b4[None, :, None]
    b64 = case.b4.double()[None, :, None]
    ninf = torch.full_like(exact, -np.inf)
    live_p = (_per_pt(live) & real)[:, None, :]                                      # the item's real points
    final = torch.relu(torch.where(live_p.expand_as(exact), exact, ninf).amax(2) + b64[:, :, 0])   # (B,512) float64
    arg = torch.where(live_p.expand_as(exact), exact, ninf).argmax(2)               # (B,512)

    # the slot map of every item: round_of (B,nt), -1 where the tile is not live
    round_of = torch.full((B, nt), -1, dtype=torch.int64)
    visits = torch.zeros((B, nt), dtype=torch.int64)
    n_rounds = 0
    for b in range(B):
        for r, tiles in enumerate(slot_map(int(case.n_live[b]))):
            assert 1 <= len(tiles) <= WAVES, (case.what, b, r, "a round holds one to four tiles")
            for t in tiles:
                round_of[b, t] = r
                visits[b, t] += 1
            n_rounds = max(n_rounds, r + 1)
    assert bool((visits <= 1).all()), (case.what, "a tile is visited twice")
    assert bool((visits[live] == 1).all()), (case.what, "a tile is never visited")
    assert bool((round_of[:, 0] == 0).all()), (case.what, "tile 0 is not in round 0")

    # round 0's bound phase on the round's own screened tiles, real points only
    first = (round_of == 0) & ~case.range_dense                                     # (B,nt)
    m = torch.where((_per_pt(first) & real)[:, None, :].expand_as(s16), s16, torch.full_like(s16, -np.inf))
    m = m.view(B, 512, nt, TILE).amax(-1)                                           # (B,512,nt)
    y = torch.where(first[:, None, :].expand_as(m), bound_phase(m, E, b32), torch.full_like(m, -np.inf))
    G0 = torch.relu(y.amax(2))                                                      # (B,512) fp32; -inf -> 0
    G = G0.double()

    Ep = _per_pt(E)
    cand = torch.zeros_like(live_p.expand_as(s16))
    per_round, tiles_round, over_cap, c_tile_all = [], [], 0, []
    for r in range(n_rounds):
        here_t = round_of == r                                                      # (B,nt)
        assert bool((G <= final).all()), (case.what, r, "the threshold table is above the dense result")
        G32 = G.float()[:, :, None]                        # (the 2^-22 term of thr covers this rounding)
        thr = (G32 - b32) - ((G32.abs() + b32.abs()) * f(2.0 ** -22) + Ep)
        scr_t = here_t & ~case.range_dense
        c = (s16 > thr) & (_per_pt(scr_t) & real)[:, None, :]
        c_tile = c.view(B, 512, nt, TILE).sum((1, 3))                               # (B,nt)
        over = scr_t & (c_tile > H.SCR_CAP)                                         # the list overflows: the tile is dense
        over_cap += int(over.sum())
        scr_t = scr_t & ~over
        c = c & _per_pt(scr_t)[:, None, :]
        dense_p = (_per_pt(here_t & ~scr_t) & real)[:, None, :]
        skipped = (~c & (_per_pt(scr_t) & real)[:, None, :]).expand_as(exact)
        assert bool(((exact + b64)[skipped] <= G[:, :, None].expand_as(exact)[skipped]).all()), (case.what, r, "a skipped pair could raise the result")
        in_round = (_per_pt(here_t) & real).gather(1, arg.view(B, -1)).view(B, 512)  # the item's fp32 arg-max lies in this round
        covered = (c | dense_p.expand_as(c)).gather(2, arg[:, :, None])[:, :, 0]
        ok = covered | (G >= final) | ~in_round
        assert bool(ok.all()), (case.what, r, "the fp32 arg-max is not a candidate and G is below the final value")
        cand |= c
        n_scr = int(scr_t.sum())
        per_round.append(float(c.sum()) / max(1, n_scr))
        tiles_round.append(n_scr)
        c_tile_all.append(c_tile[scr_t])
        # the round's exact values: candidates, and every point of a dense tile
        took = c | dense_p.expand_as(c)
        G = torch.maximum(G, torch.relu(torch.where(took, exact + b64, ninf).amax(2)))
    assert bool((G == final).all()), (case.what, "the item's table is not the dense result after the last round")
    ct = torch.cat(c_tile_all).double() if c_tile_all else torch.zeros(0, dtype=torch.float64)
    rounds_b = -(-case.n_live // WAVES)
    rep = {"what": case.what, "rounds": n_rounds, "live_tiles": int(live.sum()), "live_per_item": float(case.n_live.double().mean()),
           "tiles_dense_for_range": int(case.range_dense.sum()), "tiles_over_cap": over_cap,
           "per_tile_mean": float(ct.mean()) if ct.numel() else 0.0, "per_tile_max": int(ct.max()) if ct.numel() else 0,
           "per_round": [round(v, 1) for v in per_round], "tiles_per_round": tiles_round,
           "idle_wave_rounds": 1.0 - float(live.sum()) / float(WAVES * rounds_b.sum())}
    return cand, G0, rep


def judge(case, slot_map=slot_map, bound_phase=bound_phase):
    """-> None if the variant keeps every promise on `case`, else the reason it was rejected"""
    try:
        run(case, slot_map, bound_phase)
    except AssertionError as e:
        return str(e.args[0] if e.args else e)
    return None
