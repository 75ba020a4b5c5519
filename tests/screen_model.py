"""tests/screen_model.py — a CPU MODEL of the screened conv5 of the fp32 encoder (csrc/dal3_enc_screen.hip; test
infrastructure, numpy/torch, in the style of tests/emu16.py).

The encoder keeps of conv5's 1024 x N outputs per crop only the channel maxima. The kernels evaluate conv5 on the fp16
MFMA (operands rounded to fp16, products summed in fp32 in an order nobody specifies), bound the distance of that score
s16 to the dense kernel's value chain32 (a k-ordered fp32 fmaf chain) by eps, and recompute exactly only the pairs
(channel, point) that can still be the arg-max. This module restates the bound and both candidate rules on the oracle's
layers so that a wrong bound is found without a GPU:

  eps_l2(c,p) = KAPPA * ||w_c||_2 ||x_p||_2,   eps_l1(c,p) = KAPPA * sum_k |w_ck| |x_pk|      (the two bounds
  KAPPA       = 1.02 * 2^-10 + K * 2^-23,  K = 128                                              of the issue's table)
  E(c, wave)  = X * P_c + Q_c,  X = max ||x_p||_2 over the wave's 64 points                      (what the kernels evaluate:
  P_c = KAPPA ||w_c||_2 + 2^-24 sqrt(K),  Q_c = 2^-24 ||w_c||_1 + 2^-40                           dal3_misc.hip, bound_coefficients)

float64 on the fp32 operands stands in for the exact chain; the chain's own rounding (<= K 2^-24 sum|w||x|) is part of KAPPA.
"""
import numpy as np
import torch

import bound_model
from bound_model import fold as _fold

K = 128
KAPPA = bound_model.kappa(K)
WAVE_POINTS = 64                                          # DAL3_ENC_T = 2 tiles of 32 points per wave
F16_GUARD = 60000.0                                       # activations above this: the wave takes the dense layer
SCR_CAP = 1024                                            # candidate entries per wave and 32-point tile


def activations(sd, pts, p="ins_seg"):
    """pts (B,Cin,N) fp32 -> conv4's output x4 (B,128,N) fp32 and conv5's folded (w5 (1024,128), b5 (1024,))"""
    x = pts
    for layer, bn in (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3"), ("conv4", "bn4")):
        w, b = _fold(sd, p, layer, bn)
        x = torch.relu(torch.einsum("oc,bcn->bon", w, x) + b[None, :, None])
    w5, b5 = _fold(sd, p, "conv5", "bn5")
    return x, w5, b5


def scores(w5, x4):
    """s16 (fp16 operands, fp32 accumulate) and the exact chain's stand-in (float64 on the fp32 operands), (B,1024,N)"""
    s16 = torch.einsum("oc,bcn->bon", w5.half().float(), x4.half().float()).double()
    exact = torch.einsum("oc,bcn->bon", w5.double(), x4.double())
    return s16, exact


def eps_point(w5, x4, bound):
    """the issue's two per-pair bounds, (B,1024,N) float64"""
    w, x = w5.double(), x4.double()
    if bound == "l2":
        return KAPPA * w.norm(dim=1)[None, :, None] * x.norm(dim=1)[:, None, :]
    return KAPPA * torch.einsum("oc,bcn->bon", w.abs(), x.abs())


def coefficients(w5):
    return bound_model.coefficients(w5, K)


def _waves(t, N):
    """(..., N) -> (..., waves, 64), the ragged end filled with the crop's last point as the kernels do"""
    pad = (-N) % WAVE_POINTS
    if pad:
        t = torch.cat([t, t[..., -1:].expand(*t.shape[:-1], pad)], -1)
    return t.reshape(*t.shape[:-1], -1, WAVE_POINTS)


def eps_wave(w5, x4):
    """E(c, wave) as the kernels evaluate it, IN FP32 with their margins (dal3_enc_screen.hip: X = sqrtf(max sum x^2) *
    (1 + 2^-16); E = fmaf(X, P, Q); E = fmaf(E, 2^-20, E); P, Q rounded from double with 1e-6), broadcast to (B,1024,N)
    float32; `dense`: (B,N) points whose wave leaves the screen. (torch has no fused multiply-add: each fmaf is modelled
    with two roundings, which the margins cover as well.)"""
    B, _, N = x4.shape
    x = x4.float()
    ss = _waves((x * x).sum(1), N).amax(-1)                # (B, waves) fp32
    X = torch.sqrt(ss) * torch.tensor(1.0 + 2.0 ** -16, dtype=torch.float32)
    dense_w = _waves(x.amax(1), N).amax(-1) > F16_GUARD
    P, Q = (t.float() for t in coefficients(w5))
    E = X[:, None, :] * P[None, :, None] + Q[None, :, None]                      # (B,1024,waves) fp32
    E = E * torch.tensor(2.0 ** -20, dtype=torch.float32) + E
    spread = lambda t: t.unsqueeze(-1).expand(*t.shape, WAVE_POINTS).reshape(*t.shape[:-1], -1)[..., :N]
    return spread(E), spread(dense_w)


def table_rule(s16, eps):
    """the issue's table: candidate iff s16 + eps >= max_p (s16 - eps)"""
    L = (s16 - eps).amax(2, keepdim=True)
    return s16 + eps >= L


def kernel_rule(s16, E, b5, dense):
    """the kernels' two passes in THEIR fp32 arithmetic. s16, E: (B,1024,N) float32. Pass A, per wave: m = max_p s16,
    y = m - fmaf(|m|, 2^-22, E), g <- max(g, relu(y + b)) (a dense wave writes exact values: left out here, which only
    lowers G). Pass B: thr = (G - b) - fmaf(|G| + |b|, 2^-22, E), candidate iff s16 > thr.
    Returns (candidates (B,1024,N) bool, G (B,1024) float32)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    B, C, N = s16.shape
    b = b5.float()[None, :, None]
    live = ~dense[:, None, :].expand_as(s16)
    m = _waves(torch.where(live, s16, torch.full_like(s16, -np.inf)), N).amax(-1)             # (B,1024,waves)
    Ew = _waves(E, N)[..., 0]
    y = m - (m.abs() * f(2.0 ** -22) + Ew)
    G = torch.relu((y + b).amax(2))                                                            # -inf + b = -inf -> 0
    Gb = G[:, :, None]
    thr = (Gb - b) - ((Gb.abs() + b.abs()) * f(2.0 ** -22) + E)
    return (s16 > thr) & live, G


def check(w5, b5, x4, what=""):
    """the properties the proof gives, on one batch; returns the report"""
    s16, exact = scores(w5, x4)
    s16_f32 = s16.float()                                  # (scores() widens an fp32 einsum: this is exact)
    E32, dense = eps_wave(w5, x4)
    E = E32.double()
    live = ~dense[:, None, :].expand_as(s16)
    # points of a wave that leaves the screen (activations beyond fp16: s16 is Inf / NaN there) are the dense layer's
    ninf = torch.full_like(s16, -np.inf)
    s16, exact = torch.where(live, s16, ninf), torch.where(live, exact, ninf)
    err = torch.where(live, (s16 - exact).abs(), torch.zeros_like(s16))
    out = {"what": what}
    for bound in ("l2", "l1"):
        eps = eps_point(w5, x4, bound)
        ratio = float((err / eps.clamp_min(1e-300)).max())
        cand = table_rule(s16, eps)
        arg = exact.argmax(2, keepdim=True)
        assert ratio <= 1.0, (what, bound, "true error / eps", ratio)
        assert bool(cand.gather(2, arg).all()), (what, bound, "the fp32 arg-max is not a candidate")
        per = cand.sum(2).double()
        out[bound] = {"cand_mean": float(per.mean()), "cand_max": int(per.max()), "err_over_eps": ratio}
    ratio = float((err / E).max())
    assert ratio <= 1.0, (what, "wave bound: true error / E", ratio)
    cand, G = kernel_rule(s16_f32, E32, b5, dense)
    G = G.double()
    b = b5.double()[None, :, None]
    # pass A's value is a lower bound of the dense result; a pair that is not a candidate (and not in a dense wave) cannot raise g
    final = torch.relu(exact.amax(2) + b[:, :, 0])
    assert bool((G <= final).all()), (what, "pass A's lower bound is above the dense result")
    skipped = ~cand & ~dense[:, None, :]
    assert bool(((exact + b)[skipped] <= G[:, :, None].expand_as(exact)[skipped]).all()), (what, "a skipped pair could raise g")
    B, _, N = x4.shape
    pad = (-N) % 32
    c32 = torch.nn.functional.pad(cand, (0, pad)).view(B, 1024, -1, 32).sum((1, 3))        # candidates per 32-point tile
    per = cand.sum(2).double()
    out["kernel"] = {"cand_mean": float(per.mean()), "cand_max": int(per.max()), "err_over_E": ratio,
                     "per_tile_mean": float(c32.double().mean()), "per_tile_max": int(c32.max()),
                     "tiles_over_cap": float((c32 > SCR_CAP).double().mean()), "dense_points": float(dense.double().mean())}
    # per (crop, channel): candidates, max chain + b, the largest bound of the crop's live waves
    out["_cand"], out["_top"], out["_emax"] = cand.sum(2), exact.amax(2) + b[:, :, 0], torch.where(live, E, torch.zeros_like(E)).amax(2)
    return out
