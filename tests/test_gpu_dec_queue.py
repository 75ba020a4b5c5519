"""The row queue of the fp32 throughput decoder's compacted body (csrc/dal3_pointmlp.hip, DESIGN.md "Compacted dconv2 -
dconv4") gives the dense decoder's BITS: dconv3 and dconv4 run on the live rows of their inputs only.

The pattern of tests/test_gpu_dec_sparse.py: one launch through the throughput family against the same crops in chunks of
at most 512 tiles through the latency family (dense, untouched), `torch.equal` on the bit patterns of the logits and the
mask of every row. 24 crops x 1024 points (768 tiles) unless stated otherwise. Every case forces the compacted body with a
-1e6 shift on 200 entries of dbn1.bias, so it does not depend on the weights' own per-crop term."""
import numpy as np
import pytest
import torch

from _common import build_model, synth
from test_gpu_dec_sparse import _blob, _check, _guard_flag

pytestmark = pytest.mark.gpu

B, N = 24, 1024
GROUP = 4                                                  # dconv1 chunks (of 32 channels) per group in case (b)


def _forced(seed, kind="static_one", dbn1=None):
    """synth weights whose dconv1 term is negative in >= 200 of 512 channels for every crop (dbn1: the full shift instead)"""
    sd = dict(synth.state_dict(kind, seed=seed))
    if dbn1 is None:
        dbn1 = np.zeros(512)
        dbn1[np.random.default_rng(seed).permutation(512)[:200]] = -1e6
    sd["ins_seg.dbn1.bias"] = np.asarray(sd["ins_seg.dbn1.bias"]).astype(np.float32) + dbn1.astype(np.float32)
    return sd


def _shift(sd, bn, shift):
    sd[f"ins_seg.{bn}.bias"] = np.asarray(sd[f"ins_seg.{bn}.bias"]).astype(np.float32) + shift.astype(np.float32)
    return sd


def _run(sd, what, seed, pts=None, c_in=3, flag=0):
    model = build_model("static_one" if c_in == 3 else "dynamic", sd)
    assert _guard_flag(_blob(model)) == flag, what
    if pts is None:
        pts = synth.static_crops(B, N, seed=seed)[0]
    return _check(model, torch.from_numpy(pts).cuda(), c_in, what)


def test_a_synth_weights_as_they_are():
    lg, _ = _run(_forced(41), "synth", 41)
    assert bool(torch.isfinite(lg).all())


def _dconv1_sets():
    rng = np.random.default_rng(42)
    odd = np.full(512, -1e6)                               # every group of GROUP chunks keeps an odd count: 1, 33, 65, 127
    for g, n in enumerate((1, 33, 65, 127)):
        odd[128 * g + rng.permutation(128)[:n]] = 1e6
    dead = np.full(512, 1e6)                               # one whole group dead (256 live: the others)
    dead[128:256] = -1e6
    dead[rng.permutation(512)[:140]] = -1e6
    live = np.full(512, -1e6)                              # one whole group live, nothing else
    live[256:384] = 1e6
    first, last = np.full(512, -1e6), np.full(512, -1e6)
    first[0] = 1e6
    last[511] = 1e6
    return {"odd per group": odd, "dead group": dead, "live group": live, "only 0": first, "only 511": last}


@pytest.mark.parametrize("name", list(_dconv1_sets()))
def test_b_dconv1_live_sets(name):
    """dconv2's input: live sets chosen with +-1e6 shifts on dbn1.bias (every set has >= 200 dead channels)"""
    shift = _dconv1_sets()[name]
    assert int((shift < 0).sum()) >= 200
    _run(_forced(42, dbn1=shift), f"dconv1 {name}", 42)


def _layer_sets(c):
    """live sets of a c-channel layer input, as +-1e6 shifts: channel c - 1 is the last chain index, channel 0 the first"""
    rng = np.random.default_rng(c)
    odd = np.full(c, -1e6)
    odd[rng.permutation(c)[:c // 3 | 1]] = 1e6
    first, last = np.full(c, -1e6), np.full(c, -1e6)
    first[0] = 1e6
    last[c - 1] = 1e6
    return {"all dead": np.full(c, -1e6), "none dead": np.full(c, 1e6), "first only": first, "last only": last, "odd": odd}


@pytest.mark.parametrize("name", list(_layer_sets(256)))
def test_c_dconv3_input_sets(name):
    _run(_shift(_forced(43), "dbn2", _layer_sets(256)[name]), f"dconv3 input {name}", 43)


@pytest.mark.parametrize("name", list(_layer_sets(128)))
def test_d_dconv4_input_sets(name):
    _run(_shift(_forced(44), "dbn3", _layer_sets(128)[name]), f"dconv4 input {name}", 44)


@pytest.mark.parametrize("layer,bn_in,c", [("dconv3", "dbn2", 256), ("dconv4", "dbn3", 128)])
def test_e_infinite_weight_sets_the_flag(layer, bn_in, c):
    """an Inf weight on an input channel that is dead in every tile: the dense chain computes 0 * Inf = NaN where a body that
    skipped the row would not (the ReLU that follows works on the bit pattern and may turn that NaN into +0 again, so no
    NaN is asserted on the logits). The flag sends every tile to the dense body."""
    shift = np.zeros(c)
    shift[5] = shift[c - 2] = -1e6
    sd = _shift(_forced(45), bn_in, shift)
    wt = np.asarray(sd[f"ins_seg.{layer}.weight"]).astype(np.float32).copy()
    wt[3, 5, 0] = np.inf
    wt[100, c - 2, 0] = -np.inf
    sd[f"ins_seg.{layer}.weight"] = wt
    _run(sd, f"Inf {layer} weight", 45, flag=1)


@pytest.mark.parametrize("layer,bn", [("dconv3", "dbn3"), ("dconv4", "dbn4")])
def test_e_minus_zero_bias_sets_the_flag(layer, bn):
    sd = _forced(46)
    gamma = np.asarray(sd[f"ins_seg.{bn}.weight"]).astype(np.float32).copy()
    beta = np.asarray(sd[f"ins_seg.{bn}.bias"]).astype(np.float32).copy()
    bias = np.asarray(sd[f"ins_seg.{layer}.bias"]).astype(np.float32).copy()
    gamma[5] = -abs(gamma[5]) - np.float32(0.1)            # (b - mean) * s + beta = (+0) * (negative) + (-0) = -0
    beta[5] = np.float32(-0.0)
    bias[5] = np.asarray(sd[f"ins_seg.{bn}.running_mean"])[5]
    sd[f"ins_seg.{bn}.weight"], sd[f"ins_seg.{bn}.bias"], sd[f"ins_seg.{layer}.bias"] = gamma, beta, bias
    _run(sd, f"-0 {layer} bias", 46, flag=1)


@pytest.mark.parametrize("b,n", [(17, 1023), (520, 33)])
def test_f_ragged_tiles(b, n):
    """a last tile that replicates the crop's last point; waves of a workgroup without a tile"""
    _run(_forced(47), f"ragged {b}x{n}", 47, pts=synth.static_crops(b, n, seed=n)[0])


def test_f_crop_with_a_nan_coordinate():
    pts = synth.static_crops(B, N, seed=48)[0].copy()
    pts[3, 700, 1] = np.nan
    lg, mk = _run(_forced(48), "NaN crop", 48, pts=pts)
    good = [b for b in range(B) if b != 3]
    assert bool(torch.isnan(lg[3]).all()) and int(mk[3].sum()) == 0 and bool(torch.isfinite(lg[good]).all())


def test_g_four_input_channels():
    """c_in = 4: DynamicModel's segmentation net, 4 items x 5120 points (640 tiles)"""
    p = synth.dynamic_items(4)[0]
    _run(_forced(49, kind="dynamic"), "dynamic", 49, pts=p, c_in=4)
