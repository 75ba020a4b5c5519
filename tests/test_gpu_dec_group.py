"""dconv2's grouped consumer in the fp32 throughput decoder's compacted body (csrc/dal3_pointmlp.hip, DESIGN.md "Compacted
dconv2 - dconv4") gives the dense decoder's BITS: dconv1's chunks go to the row queue and ONE compact loop runs per group of
DAL3_DEC_GROUP chunks, an odd leftover waiting in a row of its own.

The pattern of tests/test_gpu_dec_queue.py: one launch through the throughput family against the same crops in chunks of
at most 512 tiles through the latency family (dense, untouched), `torch.equal` on the bit patterns of the logits and the
mask of every row. 24 crops x 1024 points (768 tiles) unless stated otherwise. The live sets are +-1e6 shifts on
dbn1.bias, chosen in chain order for the shipped group size (tests/dec_group_model.py::live_sets, the sets of the CPU
model's test); every one of them has at least 200 channels at -1e6, so the compacted body is taken."""
import os
import re

import numpy as np
import pytest
import torch

from _common import build_model, synth
from dec_group_model import live_sets
from dec_queue_model import chain
from test_gpu_dec_sparse import _blob, _check, _guard_flag

pytestmark = pytest.mark.gpu

B, N = 24, 1024
_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dal_pytorch_amd", "csrc", "dal3_pointmlp.hip")
GROUP = int(re.search(r"^#define DAL3_DEC_GROUP (\d+)", open(_SRC).read(), re.M).group(1))      # the shipped group
SETS = live_sets(GROUP)


def _forced(seed, kind="static_one", live=None):
    """synth weights with dconv1's term at +1e6 on the live chain indices and -1e6 on the others (live None: -1e6 on 200
    channels, the others as they are)"""
    sd = dict(synth.state_dict(kind, seed=seed))
    if live is None:
        shift = np.zeros(512)
        shift[np.random.default_rng(seed).permutation(512)[:200]] = -1e6
    else:
        shift = np.full(512, -1e6)
        shift[chain(512)[np.nonzero(live)[0]]] = 1e6
        assert int((shift < 0).sum()) >= 200
    sd["ins_seg.dbn1.bias"] = np.asarray(sd["ins_seg.dbn1.bias"]).astype(np.float32) + shift.astype(np.float32)
    return sd


def _run(sd, what, seed, pts=None, c_in=3, flag=0):
    model = build_model("static_one" if c_in == 3 else "dynamic", sd)
    assert _guard_flag(_blob(model)) == flag, what
    if pts is None:
        pts = synth.static_crops(B, N, seed=seed)[0]
    return _check(model, torch.from_numpy(pts).cuda(), c_in, what)


@pytest.mark.parametrize("name", list(SETS))
def test_a_live_sets_of_the_shipped_group(name):
    """an odd count in every group; a leftover that waits through dead groups while their rows are written over its own; the
    last chain index of a group with the first of the next; only channel 0, only 511, nothing; the longest list"""
    _run(_forced(51, live=SETS[name]), f"group {GROUP}: {name}", 51)


def test_b_synth_weights_as_they_are():
    """no forced shift: the weights' own per-crop term decides which body a tile takes"""
    lg, _ = _run(dict(synth.state_dict("static_one", seed=41)), "synth, unforced", 41)
    assert bool(torch.isfinite(lg).all())


@pytest.mark.parametrize("b,n", [(17, 1023), (520, 33)])
def test_c_ragged_tiles(b, n):
    """a last tile that replicates the crop's last point; waves of a workgroup without a tile"""
    _run(_forced(52), f"ragged {b}x{n}", 52, pts=synth.static_crops(b, n, seed=n)[0])


def test_c_crop_with_a_nan_coordinate():
    pts = synth.static_crops(B, N, seed=53)[0].copy()
    pts[3, 700, 1] = np.nan
    lg, mk = _run(_forced(53), "NaN crop", 53, pts=pts)
    good = [b for b in range(B) if b != 3]
    assert bool(torch.isnan(lg[3]).all()) and int(mk[3].sum()) == 0 and bool(torch.isfinite(lg[good]).all())


def test_d_four_input_channels():
    """c_in = 4: DynamicModel's segmentation net, 4 items x 5120 points (640 tiles)"""
    p = synth.dynamic_items(4)[0]
    _run(_forced(54, kind="dynamic"), "dynamic", 54, pts=p, c_in=4)


def test_e_infinite_dconv2_weight_sets_the_flag():
    """an Inf weight on an input channel that is dead in every tile: 0 * Inf = NaN in the dense chain, which a body that
    skipped the row would lose. The flag sends every tile to the dense body."""
    live = np.ones(512, bool)
    live[np.random.default_rng(55).permutation(512)[:220]] = False
    dead_ch = int(chain(512)[np.nonzero(~live)[0][0]])
    sd = _forced(55, live=live)
    wt = np.asarray(sd["ins_seg.dconv2.weight"]).astype(np.float32).copy()
    wt[3, dead_ch, 0] = np.inf
    sd["ins_seg.dconv2.weight"] = wt
    _run(sd, "Inf dconv2 weight", 55, flag=1)


def test_e_minus_zero_dconv2_bias_sets_the_flag():
    sd = _forced(56)
    gamma = np.asarray(sd["ins_seg.dbn2.weight"]).astype(np.float32).copy()
    beta = np.asarray(sd["ins_seg.dbn2.bias"]).astype(np.float32).copy()
    bias = np.asarray(sd["ins_seg.dconv2.bias"]).astype(np.float32).copy()
    gamma[5] = -abs(gamma[5]) - np.float32(0.1)            # (b - mean) * s + beta = (+0) * (negative) + (-0) = -0
    beta[5] = np.float32(-0.0)
    bias[5] = np.asarray(sd["ins_seg.dbn2.running_mean"])[5]
    sd["ins_seg.dbn2.weight"], sd["ins_seg.dbn2.bias"], sd["ins_seg.dconv2.bias"] = gamma, beta, bias
    _run(sd, "-0 dconv2 bias", 56, flag=1)
