"""fp32 subnormals in the screened encoder and the compacted decoder: the VALU chain, the MFMA and float64 agree where
partial sums are subnormal, and a subnormal activation is "live".

tests/test_gpu_enc_screen.py stops at coordinates x 1e-6 and conv5 x 1e-3, thirty orders of magnitude above the first fp32
subnormal; the compacted decoder tests liveness as `bits != 0` and nothing held a subnormal activation to it. A
flush-to-zero anywhere fails here even if both kernel families flush alike: every case is also held to float64
(tests/f64_ref.py), in which 2^-149 x 2^-... is an ordinary number."""
import importlib

import numpy as np
import pytest
import torch

import f64_ref as F
import f64_rows as W
from _common import build_model, synth
from oracle import ref_heads as R
from test_gpu_dec_sparse import _blob, _guard_flag
from test_gpu_enc_screen import _check, _forward
from test_gpu_f64_parity import _record_file, hold      # noqa: F401 (the fixture writes this module's rows too)

hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu

B, N, K = 96, 1024, 128
TINY = np.float32(2.0 ** -130)
ULP = 2.0 ** -149                                          # the spacing of the fp32 subnormals
MIN_NORMAL = 2.0 ** -126
SCR_CAP = 1024                                             # csrc/dal3_enc_screen.hip
FORTY = 7 + 25 * np.arange(40)
ROWS = np.asarray(W.BIG_ROWS)                              # the crops held to float64 (g of a crop needs only its points)


def _f32(sd, key):
    return np.asarray(sd[key]).astype(np.float32).copy()


def _tiny_conv5(seed, ch, cols=slice(None), unit_bn=True):
    """synth weights whose conv5 rows `ch` are scaled by 2^-130 in the input columns `cols`. unit_bn: those channels get
    conv5.bias = bn5.running_mean = 0, bn5.bias = 0 and gamma = 1 over a variance with fl(var + 1e-5f) = 1, so the fold
    (csrc/dal3_misc.hip) is exact: scale 1, bias +0 — the kernels and float64 then sum the very same subnormal weights
    (a fold that rounds a subnormal weight loses up to 2^-150 per term, which the bound below has no room for; and a mean
    of ordinary size would swallow a sum of 2^-130 in the unfolded float64 oracle)"""
    sd = dict(synth.state_dict("static_one", seed=seed))
    w = _f32(sd, "ins_seg.conv5.weight")
    w[ch, cols] = w[ch, cols] * TINY
    sd["ins_seg.conv5.weight"] = w
    if unit_bn:
        var = np.float32(1) - np.float32(1e-5)
        assert var + np.float32(1e-5) == np.float32(1)
        for key, v in (("conv5.bias", 0), ("bn5.running_mean", 0), ("bn5.bias", 0), ("bn5.weight", 1), ("bn5.running_var", var)):
            a = _f32(sd, "ins_seg." + key)
            a[ch] = v
            sd["ins_seg." + key] = a
    return sd


def _positive_channels(seed, pts_np, n):
    """the first n of every fourth channel whose float64 maximum is positive in each judged crop once the row is scaled (x4
    is non-negative and its points share a large common part, so a row's sums are negative in every point of a crop for
    about one channel in seven: such a channel pools +0 and never shows a subnormal)"""
    pool = np.arange(0, 1024, 4)
    ref = F.truth("ins_seg", _tiny_conv5(seed, pool), (torch.from_numpy(pts_np[ROWS]).transpose(2, 1),))["g"][:, pool]
    ok = pool[(ref > 0).all(0)]
    assert len(ok) >= n
    return ok[:n]


def _subnormal_sums(seed, n):
    """D1 / D2: conv5 sums that are subnormal from the first term to the last, in n channels"""
    pts_np, _, _ = synth.static_crops(B, N, seed=seed)
    ch = _positive_channels(seed, pts_np, n)
    sd = _tiny_conv5(seed, ch)
    # fp16 rounds those weights to 0: the screen's score is 0, pass A leaves G = +0, the threshold is negative, and every
    # point of those channels is a candidate — 32 per channel and tile on top of the ordinary ones
    assert not np.asarray(sd["ins_seg.conv5.weight"])[ch].astype(np.float16).any()
    model = build_model("static_one", sd)
    g = _check(model, torch.from_numpy(pts_np).cuda(), 3, f"{len(ch)} subnormal channels").cpu().numpy()   # (a)
    bits = g[:, ch].view(np.uint32)
    sub = (bits != 0) & ((bits >> 23) & 0xFF == 0)
    print(f"{len(ch)} channels: subnormal non-zero g in {sub.sum(0).min()} .. {sub.sum(0).max()} of {B} crops per channel, "
          f"g there {g[:, ch][sub].min():.3g} .. {g[:, ch][sub].max():.3g}")
    assert sub.any(0).all(), "(b) a scaled channel has no subnormal, non-zero maximum: the regime was not reached"
    ref = F.truth("ins_seg", sd, (torch.from_numpy(pts_np[ROWS]).transpose(2, 1),))["g"][:, ch]
    assert (ref > 0).all() and (ref < 4 * MIN_NORMAL).all()
    err = np.abs(g[ROWS][:, ch].astype(np.float64) - ref).max() / ULP
    # each of the K fmas rounds to the subnormal grid, error <= 2^-150; x4's own fp32 rounding is 1e-6 of a value < 2^-126
    print(f"max |g - float64| = {err:.2f} x 2^-149 (bound {K / 2 + 2:g})")
    assert err <= K / 2 + 2, "(c)"


def test_subnormal_conv5_sums_through_the_valu_recompute():
    """8 channels: 256 extra candidates per tile, below SCR_CAP with the ordinary ones (426 at most in the CPU model)"""
    assert 32 * 8 + 426 < SCR_CAP
    _subnormal_sums(61, 8)


def test_subnormal_conv5_sums_through_the_mfma_fallback():
    """40 channels: 1280 candidates per tile exceed SCR_CAP, the wave falls back to conv_max_layer on the MFMA"""
    assert 32 * 40 > SCR_CAP
    _subnormal_sums(62, 40)


def test_partial_sums_that_start_subnormal_and_end_normal():
    """the scale on the first 64 input columns only (the first eight k-groups of the chain), the BN as it is: the sums
    start subnormal and end at ordinary size; the kernels' bits agree and those channels of g meet the ordinary bars"""
    pts_np, _, _ = synth.static_crops(B, N, seed=63)
    sd = _tiny_conv5(63, FORTY, slice(0, 64), unit_bn=False)
    model = build_model("static_one", sd)
    g = _check(model, torch.from_numpy(pts_np).cuda(), 3, "mixed").cpu().numpy()
    ins = (torch.from_numpy(pts_np[ROWS]).transpose(2, 1),)
    ref = F.truth("ins_seg", sd, ins)
    yard = F.yardstick("ins_seg", sd, ins, ref64=ref)
    cut = lambda d: {"g": d["g"][:, FORTY]}
    yard_ch = F.judge(cut(F.run("ins_seg", sd, ins, dtype=torch.float32)), cut(ref))
    assert set(yard_ch) == {"g"} and yard["g"]["n_chan"] == 1024
    hold("mixed_subnormal_96x1024", "fp32", {"g": g[ROWS][:, FORTY]}, cut(ref), yard_ch)


def _dconv1_act64(sd, pts_np, g64):
    """relu(dbn1(dconv1(cat(o2, g)))) in float64 from the oracle's own layer function"""
    with F._float64_everywhere():
        tsd = {k: F._cast(v, torch.float64) for k, v in sd.items()}
        x = torch.from_numpy(pts_np).transpose(2, 1).double()
        o2 = R._cbr(tsd, "ins_seg", "conv2", "bn2", R._cbr(tsd, "ins_seg", "conv1", "bn1", x))
        cat = torch.cat([o2, torch.from_numpy(g64)[:, :, None].repeat(1, 1, x.shape[2])], 1)
        return R._cbr(tsd, "ins_seg", "dconv1", "dbn1", cat).numpy()


def _subnormal_live_setup(seed, ch, dead):
    """-> (weights, the same with dconv2's columns `ch` zeroed): dconv1's channels `dead` far below zero, the channels `ch`
    (rows, conv bias, BN mean and BN bias) scaled by 2^-130 after 3 was added to their bias, dconv2's columns `ch` by 2^120"""
    shift = np.zeros(512)
    shift[dead] = -1e6
    shift[ch] = 3.0
    sd = W.with_dconv1_bias(seed, shift)
    for key in ("dconv1.weight", "dconv1.bias", "dbn1.running_mean", "dbn1.bias"):
        a = _f32(sd, "ins_seg." + key)
        a[ch] = a[ch] * TINY
        sd["ins_seg." + key] = a
    w2 = _f32(sd, "ins_seg.dconv2.weight")
    w2[:, ch] = w2[:, ch] * np.float32(2.0 ** 120)
    assert np.isfinite(w2).all()
    sd["ins_seg.dconv2.weight"] = w2
    sd0 = dict(sd)
    z = w2.copy()
    z[:, ch] = 0
    sd0["ins_seg.dconv2.weight"] = z
    return sd, sd0


def _share_subnormal(sd, pts_np, g64, ch):
    act = _dconv1_act64(sd, pts_np, g64)[:, ch]
    return ((act > 0) & (act < MIN_NORMAL)).mean((0, 2))


def test_a_subnormal_activation_is_live_in_the_compacted_decoder():
    """192 dconv1 channels dead in every point (the compacted body), four others whose activation is a positive subnormal
    and whose dconv2 column is scaled by 2^120, so their terms are visible in dconv2's sums: the logits keep the latency
    family's bits, meet the decoder's bars against float64 and differ from a run with those four columns zeroed"""
    seed = 64
    pts_np, _, _ = synth.static_crops(B, N, seed=seed)
    ins = (torch.from_numpy(pts_np[ROWS]).transpose(2, 1),)
    order = np.random.default_rng(seed).permutation(512)
    dead, pool = order[:192], np.sort(order[192:224])
    g64 = F.truth("ins_seg", synth.state_dict("static_one", seed=seed), (ins[0][:4],))["g"]       # the encoder is untouched
    share = _share_subnormal(_subnormal_live_setup(seed, pool, dead)[0], pts_np[ROWS[:4]], g64, pool)
    ch = pool[share > 0.9][:4]                              # a channel's activation depends on its own row only
    assert len(ch) == 4
    sd, sd0 = _subnormal_live_setup(seed, ch, dead)
    ref = F.truth("ins_seg", sd, ins)
    share = _share_subnormal(sd, pts_np[ROWS[:4]], ref["g"][:4], ch)
    print("channels", ch, "share of points with a positive subnormal activation:", share)
    assert (share > 0.9).all()

    model = build_model("static_one", sd)
    blob = _blob(model)
    assert _guard_flag(blob) == 0                           # finite weights, no -0 bias: the compacted route is open
    pts = torch.from_numpy(pts_np).cuda()
    lib = hip.lib()
    g = _check(model, pts, 3, "subnormal activations")      # g, logits and mask: the latency family's bits on every row
    gb = torch.empty((B, 512), device="cuda")
    hip.check(lib.dal3_ins_seg_global_bias(hip.ptr(blob), hip.F32, hip.ptr(g), B, hip.ptr(gb), hip.stream()))
    assert int((gb < 0).sum(1).min()) >= W.DEC_MIN_DEAD      # every crop's tiles take the compacted body
    _, lg, _ = _forward(blob, 3, pts.transpose(2, 1))
    lg = lg.cpu().numpy()
    yard = F.yardstick("ins_seg", sd, ins, ref64=ref)
    j = hold("subnormal_live_96x1024", "fp32", {"logits": lg[ROWS]}, ref, yard)
    _, lg0, _ = _forward(_blob(build_model("static_one", sd0)), 3, pts.transpose(2, 1))
    moved = float(np.abs(lg - lg0.cpu().numpy()).max() / np.abs(lg).max())
    print(f"zeroing the four columns moves the logits by {moved:.3g} of their maximum")
    assert moved > 10 * max(j["logits"]["tensor"], yard["logits"]["tensor"]), "the four terms are not visible above the arithmetic's error"
