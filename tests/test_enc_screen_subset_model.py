"""Pass A of the screened encoder on a SUBSET of a crop's waves (csrc/dal3_enc_screen.hip, DAL3_SCR_A_STRIDE), on the CPU.

The proof of the screen needs "G <= the final value" of pass A and nothing else, and the maximum over any subset of the
points, minus the wave's bound, is still a lower bound. This file restates pass A of tests/screen_model.py (imported
unchanged) on every S-th wave-slot of 64 points, leaves pass B's rule as it is, and asserts for S in 1, 2, 4, 8 what the
proof promises: G never exceeds the final value, a skipped pair can never raise the pooled value, and the fp32 arg-max
is a candidate unless G is the final value already. The price of a subset is candidates: the counts are printed (-s)
and, for the shipped stride, held below the list's capacity on the bench crops."""
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import screen_model as S
from _common import synth
from oracle import ref_heads as R

STRIDES = (1, 2, 4, 8)


def shipped_stride():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dal_pytorch_amd", "csrc", "dal3_enc_screen.hip")
    with open(src) as f:
        return int(re.search(r"^#define DAL3_SCR_A_STRIDE (\d+)", f.read(), re.M).group(1))


def subset_rule(s16, E, b5, dense, stride):
    """screen_model.kernel_rule with pass A restricted to the wave-slots 0, S, 2S, ... of each crop (a visited wave that
    leaves the screen contributes nothing, as there); pass B's threshold and candidate rule are unchanged and see every
    point. s16, E: (B,1024,N) float32 -> (candidates (B,1024,N) bool, G (B,1024) float32)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    N = s16.shape[2]
    b = b5.float()[None, :, None]
    live = ~dense[:, None, :].expand_as(s16)
    m = S._waves(torch.where(live, s16, torch.full_like(s16, -np.inf)), N).amax(-1)[..., ::stride]
    Ew = S._waves(E, N)[..., 0][..., ::stride]
    y = m - (m.abs() * f(2.0 ** -22) + Ew)
    G = torch.relu((y + b).amax(2))
    Gb = G[:, :, None]
    thr = (Gb - b) - ((Gb.abs() + b.abs()) * f(2.0 ** -22) + E)
    return (s16 > thr) & live, G


class Case:
    """one batch: the scores and bounds are computed once and shared by the strides"""

    def __init__(self, sd, pts_np, what):
        self.what = what
        x4, self.w5, self.b5 = S.activations(R.as_torch_sd(sd), torch.from_numpy(pts_np).transpose(2, 1))
        s16, exact = S.scores(self.w5, x4)
        self.s16 = s16.float()
        self.E, self.dense = S.eps_wave(self.w5, x4)
        live = ~self.dense[:, None, :].expand_as(exact)
        self.live = live
        self.exact = torch.where(live, exact, torch.full_like(exact, -np.inf))
        self.N = x4.shape[2]

    def check(self, stride):
        cand, G = subset_rule(self.s16, self.E, self.b5, self.dense, stride)
        G = G.double()
        b = self.b5.double()[None, :, None]
        final = torch.relu(self.exact.amax(2) + b[:, :, 0])
        assert bool((G <= final).all()), (self.what, stride, "pass A's bound is above the dense result")
        skipped = ~cand & self.live
        assert bool(((self.exact + b)[skipped] <= G[:, :, None].expand_as(self.exact)[skipped]).all()), \
            (self.what, stride, "a skipped pair could raise g")
        arg = self.exact.argmax(2, keepdim=True)
        has_live = self.live.any(2)
        ok = cand.gather(2, arg)[:, :, 0] | (G >= final) | ~has_live
        assert bool(ok.all()), (self.what, stride, "the fp32 arg-max is not a candidate and G is below the final value")
        B = cand.shape[0]
        c32 = torch.nn.functional.pad(cand, (0, (-self.N) % 32)).view(B, 1024, -1, 32).sum((1, 3))
        rep = {"what": self.what, "stride": stride, "cand_mean": float(cand.sum(2).double().mean()),
               "per_tile_mean": float(c32.double().mean()), "per_tile_p99": float(c32.double().flatten().quantile(0.99)),
               "per_tile_max": int(c32.max()), "tiles_over_cap": float((c32 > S.SCR_CAP).double().mean())}
        print(json.dumps(rep))
        return cand, rep


@functools.lru_cache(maxsize=None)
def _bench():
    return Case(synth.state_dict("static_one"), synth.static_crops(32, 1024)[0], "bench")


@pytest.mark.parametrize("stride", STRIDES)
def test_bench_crops(stride):
    """the 32 bench crops. The counts grow as order statistics say (a 1/S subset leaves about S - 1 more points above its
    maximum): they are printed, and no tile may exceed the list at the shipped stride. A larger subset gives a bound at
    least as high, so the candidates of a stride that divides another are a subset of that one's."""
    case = _bench()
    cand, rep = case.check(stride)
    if stride <= shipped_stride():
        assert rep["tiles_over_cap"] == 0.0 and rep["per_tile_max"] <= S.SCR_CAP
    if stride > 1:
        finer, _ = subset_rule(case.s16, case.E, case.b5, case.dense, stride // 2)
        assert bool((cand | ~finer).all()) and int(cand.sum()) > int(finer.sum())


def test_stride_one_is_the_model_of_the_unstrided_kernel():
    """S = 1 gives screen_model.kernel_rule's candidates pair for pair, and its counts on the bench crops: 2.66 per (crop,
    channel), 85 per 32-point tile (the margins: the rounding of those digits plus the 2 % that the free summation order
    of the CPU's matmul leaves a mean, as in tests/test_enc_screen_model.py)"""
    case = _bench()
    cand, rep = case.check(1)
    ref, G = S.kernel_rule(case.s16, case.E, case.b5, case.dense)
    assert torch.equal(cand, ref)
    assert abs(rep["cand_mean"] - 2.66) < 0.005 + 0.02 * 2.66 and abs(rep["per_tile_mean"] - 85.0) < 0.5 + 0.02 * 85.0
    assert rep["tiles_over_cap"] == 0.0


def _adversarial(pts_np):
    """the crops of tests/test_enc_screen_model.py and those a subset can get wrong (a wave-slot is 64 points; the even
    slots hold every slot that a stride of 2, 4 or 8 visits)"""
    p = pts_np.copy()
    N = p.shape[1]
    slot = np.arange(N) // S.WAVE_POINTS
    p[0, N // 2:] = p[0, :N // 2]                          # duplicated points: exact ties
    p[1, :] = p[1, 0]                                       # all points equal
    p[2] *= np.float32(1e4)                                 # coordinates of 1e4: every wave leaves the screen
    p[3] *= np.float32(1e-6)                                # ... and of 1e-6
    p[4, 200:264] *= np.float32(300.0)
    p[5, :] = 0.0
    p[6, slot % 2 == 0] = 0.0                               # the bound is useless: every visited point is the origin,
    p[6, slot % 2 == 1] *= np.float32(40.0)                 # the others are far away
    p[7, (slot >= 1) & (slot <= 3)] *= np.float32(25.0)     # the crop's largest coordinates in slots 1 to 3 only
    p[8, slot % 2 == 1] *= np.float32(1e4)                  # dense for range in unvisited slots only,
    p[9, slot % 2 == 0] *= np.float32(1e4)                  # in the visited ones only (no bound at all from pass A),
    p[10, slot == 0] *= np.float32(1e4)                     # and in slot 0 alone
    return p


@functools.lru_cache(maxsize=None)
def _adv(scale5, shift5):
    sd = dict(synth.state_dict("static_one", seed=91))
    sd["ins_seg.conv5.weight"] = (np.asarray(sd["ins_seg.conv5.weight"]) * np.float32(scale5)).astype(np.float32)
    if shift5:
        bias = np.asarray(sd["ins_seg.bn5.bias"]).astype(np.float32).copy()
        bias[::2] += np.float32(shift5)
        sd["ins_seg.bn5.bias"] = bias
    return Case(sd, _adversarial(synth.static_crops(12, 1024, seed=91)[0]), f"adversarial x{scale5:g} {shift5:+g}")


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("scale5,shift5", [(1.0, 0.0), (1e3, 0.0), (1e-3, 0.0), (1.0, -50.0)])
def test_adversarial_crops(scale5, shift5, stride):
    """ties, constant crops, huge and tiny coordinates, a useless bound, the maximum in unvisited slots, dense waves in
    the visited or the unvisited slots; conv5 scaled by 1e3 / 1e-3, channels whose maximum is negative"""
    case = _adv(scale5, shift5)
    cand, _ = case.check(stride)
    if stride > 1 and scale5 == 1.0 and not shift5:
        # crop 9: every visited wave is dense, pass A leaves G = +0, and a pair is a candidate iff its score can be positive
        _, G = subset_rule(case.s16[9:10], case.E[9:10], case.b5, case.dense[9:10], stride)
        assert float(G.max()) == 0.0 and bool(case.dense[9, :64].all()) and not bool(case.dense[9, 64:128].any())


@pytest.mark.parametrize("N", [64, 65, 300, 1000])
def test_short_and_ragged_crops(N):
    """fewer wave-slots than the stride, one slot, a slot count that is no multiple of the stride: slot 0 is always
    visited, so every crop gets a bound"""
    case = Case(synth.state_dict("static_one", seed=7), synth.static_crops(6, N, seed=N)[0], f"ragged {N}")
    for stride in STRIDES:
        case.check(stride)
