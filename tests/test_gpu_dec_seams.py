"""The layer seams of the fp32 throughput decoder's compacted body (csrc/dal3_pointmlp.hip, DESIGN.md "Compacted dconv2 -
dconv4"): the live mask of dconv3's and dconv4's input is taken one out-tile (32 chain indices, one mask word) at a time —
16 ballots collected in the lanes of one vector register, one compare per word — and the list is built from those words.
The live sets here are laid out by out-tile: a word with one bit, a full word between empty ones, the first and the last
lane of a word, halves of the layer dead, and per-tile counts that put every word's boundary at an odd running count.

The pattern of tests/test_gpu_dec_queue.py: one launch through the throughput family against the same crops in chunks of
at most 512 tiles through the latency family (dense, untouched), `torch.equal` on the bit patterns of the logits and the
mask of every row. 24 crops x 1024 points (768 tiles, the smallest launch that takes the throughput family). Every case
forces the compacted body with a -1e6 shift on 200 entries of dbn1.bias; the live sets of a layer's input are planted with
+-1e6 shifts on the BatchNorm bias of the layer that produces it."""
import numpy as np
import pytest
import torch

from _common import synth
from test_gpu_dec_queue import B, N, _forced, _run, _shift

pytestmark = pytest.mark.gpu


def _tiles(c, counts, seed=0):
    """counts[t] live channels (+1e6) in out-tile t of a c-channel layer input, every other channel dead (-1e6)"""
    assert len(counts) == c // 32
    rng = np.random.default_rng(seed)
    s = np.full(c, -1e6)
    for t, n in enumerate(counts):
        s[32 * t + rng.permutation(32)[:n]] = 1e6
    return s


def _seam_sets(c):
    nt = c // 32
    first, last = np.full(c, -1e6), np.full(c, -1e6)
    first[0] = 1e6
    last[c - 1] = 1e6
    sets = {"only 0": first, f"only {c - 1}": last, "one per out-tile": _tiles(c, [1] * nt, 1)}
    for t in (0, 3, 4, 7) if nt == 8 else (0, 1, 2, 3):
        sets[f"out-tile {t} live"] = _tiles(c, [32 if u == t else 0 for u in range(nt)])
    # the list starts with the words of the upper half / ends with those of the lower half
    sets["low half dead"] = _tiles(c, [0] * (nt // 2) + [32] * (nt // 2))
    sets["high half dead"] = _tiles(c, [32] * (nt // 2) + [0] * (nt // 2))
    # odd counts per word; the running count at the words' boundaries is 1, 4, 35, 67, 67, 72, 79, 88 (odd, even, an empty
    # word in between) | 1, 4, 35, 67 and 0, 5, 12, 21
    if nt == 8:
        sets["odd boundaries"] = _tiles(c, [1, 3, 31, 32, 0, 5, 7, 9], 2)
    else:
        sets["odd boundaries a"] = _tiles(c, [1, 3, 31, 32], 2)
        sets["odd boundaries b"] = _tiles(c, [0, 5, 7, 9], 3)
    sets["all dead"] = np.full(c, -1e6)
    sets["all live"] = np.full(c, 1e6)
    return sets


@pytest.mark.parametrize("name", list(_seam_sets(256)))
def test_a_dconv3_input_sets(name):
    _run(_shift(_forced(51), "dbn2", _seam_sets(256)[name]), f"dconv3 input {name}", 51)


@pytest.mark.parametrize("name", list(_seam_sets(128)))
def test_b_dconv4_input_sets(name):
    _run(_shift(_forced(52), "dbn3", _seam_sets(128)[name]), f"dconv4 input {name}", 52)


@pytest.mark.parametrize("bn,c", [("dbn2", 256), ("dbn3", 128)])
@pytest.mark.parametrize("which", [0, 1])
def test_c_dynamic_head_weights(bn, c, which):
    """c_in = 4: DynamicModel's segmentation net, 4 items x 5120 points (640 tiles); the first two sets of either layer"""
    name = list(_seam_sets(c))[which]
    p = synth.dynamic_items(4)[0]
    _run(_shift(_forced(53, kind="dynamic"), bn, _seam_sets(c)[name]), f"dynamic {bn} {name}", 53, pts=p, c_in=4)


def test_d_synth_weights_as_they_are():
    """nothing planted behind dconv1: the live sets of dconv3's and dconv4's inputs differ from tile to tile"""
    lg, _ = _run(_forced(54), "synth", 54)
    assert bool(torch.isfinite(lg).all())


def test_e_nonfinite_crop_between_two_good_ones():
    pts = synth.static_crops(B, N, seed=55)[0].copy()
    pts[11, 5, 2] = np.inf
    lg, mk = _run(_forced(55), "Inf crop", 55, pts=pts)
    good = [b for b in range(B) if b != 11]
    assert bool(torch.isnan(lg[11]).all()) and int(mk[11].sum()) == 0 and bool(torch.isfinite(lg[good]).all())
