"""Pass A of the screened fp32 encoder visits a SUBSET of each crop's wave-slots (csrc/dal3_enc_screen.hip,
DAL3_SCR_A_STRIDE) and pass B owns every exact value: the pooled feature still has the dense encoder's BITS.

The harness is tests/test_gpu_enc_screen.py's: one large launch (the screened pair of kernels) against the same crops in
chunks of at most 512 tiles through the latency family, `torch.equal` on the bits of g, on the logits and on the mask of
ALL rows, no tolerance. Every shape has B * tiles > 512 and B * N > 65536 (the harness asserts it). The cases put what
pass A no longer sees — the crop's maximum, the points that leave fp16's range, a non-finite coordinate — into the
wave-slots (64 consecutive points) that the shipped stride skips, and make crops with fewer slots than the stride."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from _common import build_model, synth
from test_gpu_enc_screen import _check

pytestmark = pytest.mark.gpu
SLOT = 64                                                   # DAL3_ENC_T = 2 tiles of 32 points per wave


@functools.lru_cache(maxsize=None)
def _stride():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dal_pytorch_amd", "csrc", "dal3_enc_screen.hip")
    with open(src) as f:
        return int(re.search(r"^#define DAL3_SCR_A_STRIDE (\d+)", f.read(), re.M).group(1))


def _visited(N):
    """(N,) bool: the points of the wave-slots 0, S, 2S, ... (with S = 1 every case below degenerates and still must hold)"""
    return (np.arange(N) // SLOT) % _stride() == 0


@functools.lru_cache(maxsize=None)
def _model(seed=None, scale5=1.0):
    sd = dict(synth.state_dict("static_one") if seed is None else synth.state_dict("static_one", seed=seed))
    if scale5 != 1.0:
        sd["ins_seg.conv5.weight"] = (np.asarray(sd["ins_seg.conv5.weight"]) * np.float32(scale5)).astype(np.float32)
    return build_model("static_one", sd)


def _run(model, p, what):
    return _check(model, torch.from_numpy(p).cuda(), 3, what)


@pytest.mark.parametrize("B,N", [(80, 1024), (260, 300), (1100, 64), (1100, 65), (140, 1000)])
def test_points_per_crop_sweep_on_bench_crops(B, N):
    """bench weights and crops; 16, 5, 1, 2 and 16 wave-slots per crop: a whole number of pass-A workgroups, fewer slots
    than the stride, one slot, a second slot of one point, a slot count that is no multiple of 4 * stride"""
    pts_np, _, _ = synth.static_crops(B, N)
    g = _run(_model(), pts_np, f"sweep {B}x{N}")
    assert bool(torch.isfinite(g).all()) and float(g.max()) > 0


def test_the_bound_is_useless():
    """in some crops every point pass A visits is a copy of the origin and the other points are scaled by 40: the bound is
    that of the origin, most tiles of those crops overflow the candidate list and take the dense layer"""
    p = synth.static_crops(96, 1024, seed=81)[0].copy()
    v = _visited(1024)
    for b in (0, 7, 31, 64, 95):
        p[b, v] = 0.0
        p[b, ~v] *= np.float32(40.0)
    _run(_model(81), p, "useless bound")


def test_the_maximum_in_an_unvisited_wave():
    """the crop's largest coordinates sit in wave-slots 1 to 3 only (with the stride at 2, slot 2 is visited: slots 1 and 3
    still hold maxima that pass A never sees)"""
    p = synth.static_crops(96, 1024, seed=82)[0].copy()
    far = (np.arange(1024) // SLOT >= 1) & (np.arange(1024) // SLOT <= 3)
    for b, k in ((1, 3.0), (8, 10.0), (33, 30.0), (70, 100.0), (94, 3.0)):
        p[b, far] *= np.float32(k)
    _run(_model(82), p, "maximum unvisited")


def test_dense_for_range_in_unvisited_visited_and_all_waves():
    """points scaled by 1e4 (activations beyond fp16's range: the wave leaves the screen) in the unvisited wave-slots
    only, in the visited ones only — pass A then has no bound at all for the crop — and in all: pass B computes those
    waves densely in all three layouts"""
    p = synth.static_crops(96, 1024, seed=83)[0].copy()
    v = _visited(1024)
    for b in (2, 40, 93):
        p[b, ~v] *= np.float32(1e4)
    for b in (3, 41, 95):
        p[b, v] *= np.float32(1e4)
    for b in (4, 42):
        p[b] *= np.float32(1e4)
    p[5, 64:128] *= np.float32(1e4)                         # one unvisited slot; one visited slot: slot 0
    p[6, 0:64] *= np.float32(1e4)
    _run(_model(83), p, "dense for range")


def test_blob_flag():
    """conv5's weights x 1e7, not finite in fp16: the blob's flag is set, pass A idles and pass B is the dense encoder"""
    p = synth.static_crops(96, 1024, seed=84)[0]
    g = _run(_model(84, 1e7), p, "blob flag")
    assert float(g.max()) > 0


def test_non_finite_crop_in_an_unvisited_wave():
    """the NaN or Inf coordinate is in a wave-slot pass A skips (slots 1, 3 and the crop's last): the crop's pooled
    feature is the quiet-NaN pattern in every channel, its neighbours are untouched"""
    B, N = 96, 1024
    pts_np, _, _ = synth.static_crops(B, N, seed=85)
    p = pts_np.copy()
    p[1, 64 + 7, 0] = np.nan
    p[3, 3 * 64, 2] = np.inf
    p[4, N - 1, 1] = -np.inf
    p[95, 127, 1] = np.nan
    g = _run(_model(85), p, "non-finite")
    bad = [1, 3, 4, 95]
    good = [b for b in range(B) if b not in bad]
    assert bool(torch.isnan(g[bad]).all()) and bool(torch.isfinite(g[good]).all())
    clean = _run(_model(85), pts_np, "clean")
    assert torch.equal(clean[good], g[good])
