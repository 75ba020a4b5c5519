"""tests/dec_prune_model.py — a CPU MODEL of the per-crop pruning of dconv1 in the fp32 throughput decoder (DESIGN.md
"Crop-dead channels of dconv1"; test infrastructure on the oracle's layers, in the style of tests/screen_model.py).

dconv1's pre-activation of channel c at point p is the decoder's k-ordered fp32 fmaf chain

    chain32(c,p) = fmaf chain over K = 64 products w_ck x2_k(p), started from gb_c

gb = W1g' g + b1' being the crop's term and x2 conv2's output. The screened encoder evaluates the products on the fp16 MFMA
while x2 is in registers and leaves per crop U_c = max_p s16(c,p) and X = max_p ||x2(p)||_2. The plan kernel flags c iff

    gb_c + U_c + E_c < 0,   E_c >= X P_c + Q_c + 2 K 2^-24 |gb_c|      (|s16 - (chain32 - gb_c)| <= that, per point)

and the decoder runs dconv1 over the unflagged channels only: their chain indices in ascending order, padded to whole
chunks of 32 with a null channel (zero weights, term -1). This module restates the bound, the plan kernel's fp32 evaluation
and the plan's layout, and holds the JUDGE that the tests turn on planted faults.
"""
import numpy as np
import torch

import bound_model
from _common import dec_min_dead
from bound_model import fold as _fold
from dec_sparse_model import fmaf, tile_chan

K = 64
KAPPA = bound_model.kappa(K)
F16_GUARD = 60000.0                                       # an x2 entry above this: the crop has no bound
NULL_K = 512                                              # DEC_NULL_K
PLAN_LD = 640                                             # DEC_PLAN_LD
MIN_DEAD = dec_min_dead()                                 # DAL3_DEC_MIN_DEAD
CHAIN = np.array([32 * c + tile_chan(r, h) for c in range(16) for r in range(16) for h in (0, 1)])   # chain index -> channel
K_ORDER = np.array([32 * kt + tile_chan(r, h) for kt in range(2) for r in range(16) for h in (0, 1)])  # dconv1's own k order
f32 = lambda v: torch.tensor(v, dtype=torch.float32)


def layers(sd, pts, p="ins_seg"):
    """pts (B,Cin,N) fp32 -> x2 (B,64,N), the crops' term gb (B,512), dconv1's folded per-point weights w1a (512,64)"""
    x = pts
    x2 = None
    for i, (layer, bn) in enumerate((("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3"), ("conv4", "bn4"), ("conv5", "bn5"))):
        w, b = _fold(sd, p, layer, bn)
        x = torch.relu(torch.einsum("oc,bcn->bon", w, x) + b[None, :, None])
        if i == 1:
            x2 = x
    g = x.amax(2)                                          # (B,1024); a NaN coordinate makes the whole row NaN on the device
    bad = ~torch.isfinite(pts).all(2).all(1)
    g[bad] = float("nan")
    w1, b1 = _fold(sd, p, "dconv1", "dbn1")
    gb = g @ w1[:, 64:].T + b1[None, :]
    return x2, gb, w1[:, :64].contiguous()


def coefficients(w1a):
    return bound_model.coefficients(w1a, K)


def scores(w1a, x2):
    """s16 (fp16 operands, fp32 accumulate), (B,512,N) float32"""
    return torch.einsum("oc,bcn->bon", w1a.half().float(), x2.half().float())


def encoder_side(w1a, x2, pts):
    """what pass B leaves per crop: U (B,512) fp32, X (B,) fp32 — +Inf for a crop without a bound (an x2 entry above the fp16
    guard, or a non-finite coordinate)"""
    ss = (x2 * x2).sum(1).amax(1)
    X = torch.sqrt(ss) * f32(1.0 + 2.0 ** -16)
    ok = (x2.amax((1, 2)) <= F16_GUARD) & torch.isfinite(pts).all(2).all(1) & torch.isfinite(x2).all(2).all(1)
    X = torch.where(ok, X, torch.full_like(X, float("inf")))
    U = scores(w1a, torch.where(ok[:, None, None], x2, torch.zeros_like(x2))).amax(2)
    return U, X


def bound(gb, X, P, Q, gb_term=True):
    """E_c as the plan kernel evaluates it, in fp32 with its margins, WITHOUT the term for the rounding of gb + U (which
    is no part of the inequality on the scores); gb_term=False is the planted fault"""
    E = X[:, None] * P.float()[None, :] + Q.float()[None, :]
    if gb_term:
        E = gb.abs() * f32(2.0 ** -17) + E
    return E * f32(2.0 ** -20) + E


def flags(gb, U, X, P, Q, gb_term=True):
    """the plan kernel's decision, every rounding against flagging; a NaN compares false"""
    E = X[:, None] * P.float()[None, :] + Q.float()[None, :]
    if gb_term:
        E = gb.abs() * f32(2.0 ** -17) + E
    t = gb + U
    E = (gb.abs() + U.abs()) * f32(2.0 ** -22) + E
    E = E * f32(2.0 ** -20) + E
    return (t + E) < 0


def chain_from_gb(w1a, gb_row, x2_crop):
    """the decoder's dconv1 accumulators of one crop: w1a (512,64), gb_row (512,), x2_crop (64,N) numpy fp32 -> (512,N)"""
    acc = np.repeat(gb_row[:, None], x2_crop.shape[1], axis=1).astype(np.float32)
    for k in K_ORDER:
        acc = fmaf(w1a[:, k][:, None], x2_crop[k][None, :], acc)
    return acc


def plan(flagged_row, gb_row):
    """flagged_row (512,) bool by CHANNEL, gb_row (512,) -> (k list (PLAN_LD,), gbc (512,), nch): the plan kernel's three
    outputs. nch = 0: fewer than MIN_DEAD flags, the crop has no plan (the other two are still written)."""
    live_k = np.array([k for k in range(512) if not flagged_row[CHAIN[k]]], np.int64)
    n = len(live_k)
    lst = np.full(PLAN_LD, NULL_K, np.int64)
    lst[:n] = live_k
    nch = 0 if 512 - n < MIN_DEAD else max(2, ((n + 31) // 32 + 1) & ~1)
    gbc = np.full(512, -1.0, np.float32)
    for j in range(16):
        for r in range(16):
            for h in (0, 1):
                k = lst[32 * j + 2 * r + h]
                if k < NULL_K:
                    gbc[32 * j + tile_chan(r, h)] = gb_row[CHAIN[k]]
    return lst, gbc, nch


def judge_bound(w1a, gb, x2, E):
    """|s16(c,p) - (chain32(c,p) - gb_c)| <= E_c at every point of every crop; returns the largest ratio. E (B,512)."""
    s16 = scores(w1a, x2).numpy()
    worst = 0.0
    for b in range(x2.shape[0]):
        ch = chain_from_gb(w1a.numpy(), gb[b].numpy(), x2[b].numpy()).astype(np.float64)
        err = np.abs(s16[b].astype(np.float64) - (ch - gb[b].numpy().astype(np.float64)[:, None])).max(1)
        ratio = float((err / E[b].numpy().astype(np.float64)).max())
        worst = max(worst, ratio)
    assert worst <= 1.0, ("the bound does not hold: error / E", worst)
    return worst


def judge_plan(lst, gbc, nch, flagged_row, gb_row):
    """the layout the decoder relies on: the unflagged chain indices, each once, ascending; null channels behind them up to
    PLAN_LD; the null channel's term negative (dead by construction: zero weights); every other term the crop's own; the
    chunk count even, at least 2, and just enough"""
    n = int((~flagged_row).sum())
    live = lst[:n]
    assert (live < NULL_K).all() and (np.diff(live) > 0).all(), "the list is not in ascending chain order"
    assert sorted(CHAIN[live]) == sorted(np.nonzero(~flagged_row)[0]), "the list is not the unflagged channels"
    assert (lst[n:] == NULL_K).all(), "behind the list: null channels only"
    for j in range(16):
        for r in range(16):
            for h in (0, 1):
                k, v = lst[32 * j + 2 * r + h], gbc[32 * j + tile_chan(r, h)]
                if k == NULL_K:
                    assert v < 0 and np.isfinite(v), "a padding entry is not dead"
                else:
                    assert v.tobytes() == np.float32(gb_row[CHAIN[k]]).tobytes(), "a term is not its channel's"
    if 512 - n < MIN_DEAD:
        assert nch == 0
    else:
        assert nch % 2 == 0 and nch >= 2 and 32 * nch >= n and (32 * (nch - 2) < n or nch == 2), ("chunk count", n, nch)
