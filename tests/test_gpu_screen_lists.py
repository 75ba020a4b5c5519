"""The candidate lists of the screened fp32 encoder (csrc/dal3_screen.h: hit words parked per block, lists built once per
wave by a prefix scan, recompute with staged weight rows) leave the dense encoder's BITS.

The inputs aim at the list building itself: points repeated 2, 4 and 8 times consecutively fall into one lane half of one
32-point tile, so a lane holds several hits of one block (the copies tie in every channel, and every copy of an arg-max
is a candidate); constant crops make every (channel, point) pair a candidate and overflow the lists (dense layer); ragged
point counts leave a partly filled last wave-slot. Every case is the smallest that still takes the throughput family's
big-job branch, and is compared on every row with `_check` of tests/test_gpu_enc_screen.py (the latency family)."""
import numpy as np
import pytest
import torch

from _common import build_model, synth
from test_gpu_enc_screen import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def static_model():
    return build_model("static_one", synth.state_dict("static_one", seed=13))


@pytest.mark.parametrize("copies", [2, 4, 8])
def test_points_repeated_consecutively(static_model, copies):
    """`copies` consecutive copies of every distinct point: 4 copies are registers 4q..4q+3 of one lane half, at least 3
    hits of a lane in the block of every channel whose maximum the point holds"""
    B, N = 80, 1024
    pts_np, _, _ = synth.static_crops(B, N // copies, seed=130 + copies)
    p = np.repeat(pts_np, copies, axis=1)
    assert p.shape == (B, N, 3)
    _check(static_model, torch.from_numpy(np.ascontiguousarray(p)).cuda(), 3, f"{copies} copies")


def test_constant_crops_overflow_the_lists_beside_range_fallbacks(static_model):
    """ten constant crops (every pair a candidate: more than SCR_CAP per tile, the dense layer) among ordinary ones and
    crops whose activations leave fp16's range (the dense layer for range)"""
    B, N = 80, 1024
    pts_np, _, _ = synth.static_crops(B, N, seed=134)
    p = pts_np.copy()
    for b in range(5, 75, 7):
        p[b, :] = p[b, b]
    p[2] *= np.float32(1e4)
    p[40, 512:] *= np.float32(1e4)
    p[77] *= np.float32(1e4)
    g = _check(static_model, torch.from_numpy(p).cuda(), 3, "constant crops")
    assert bool(torch.isfinite(g).all())


@pytest.mark.parametrize("B,N", [(1100, 65), (260, 300)])
def test_ragged_last_slot(static_model, B, N):
    """65 points: one point in the second wave-slot; 300: 44 points in the fifth"""
    pts_np, _, _ = synth.static_crops(B, N, seed=N)
    _check(static_model, torch.from_numpy(pts_np).cuda(), 3, f"ragged {B}x{N}")


def test_dynamic_weights_four_input_channels():
    p, _, _, _ = synth.dynamic_items(20)
    assert p.shape[1:] == (5120, 4)
    model = build_model("dynamic", synth.state_dict("dynamic"))
    _check(model, torch.from_numpy(p).cuda(), 4, "Dynamic_fp32 20x5120")
