"""The screened fp32 encoder (csrc/dal3_enc_screen.hip) gives the dense encoder's BITS.

The dense reference inside the library is the latency family (csrc/dal3_latency.hip), which `launch_ins_seg_encode`
takes for jobs of at most 512 tiles of 32 points and which the screen does not touch. Every case pushes one large
launch (the screened pair of kernels) and the same crops in chunks small enough for the latency family through
`dal3_ins_seg_forward`, and asserts `torch.equal` on the pooled feature of ALL rows — no sampling, no tolerance —
and on the logits and the mask that follow from it."""
import importlib

import numpy as np
import pytest
import torch

from _common import build_model, synth

hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu


def _forward(w, c_in, x):
    """x: (B, c_in, N) view on the GPU -> (global feature, logits, mask) of one dal3_ins_seg_forward launch"""
    lib = hip.lib()
    B, _, N = x.shape
    ws = torch.empty(lib.dal3_ins_seg_workspace_bytes(B), dtype=torch.uint8, device="cuda")
    g = torch.empty((B, 1024), device="cuda")
    lg = torch.empty((B, N, 2), device="cuda")
    mk = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    hip.check(lib.dal3_ins_seg_forward(hip.ptr(w), hip.F32, c_in, hip.bcn(x), B, N, hip.ptr(lg), hip.ptr(mk), hip.ptr(g),
                                       hip.ptr(ws), ws.numel(), hip.stream()))
    return g, lg, mk


def _same_bits(a, b):
    """torch.equal on the bit patterns (a NaN row equals itself)"""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check(model, pts, c_in, what):
    """pts: (B, N, c_in) on the GPU. One launch against chunks of at most 512 tiles."""
    B, N, _ = pts.shape
    tiles = (N + 31) // 32
    assert B * tiles > 512 and B * N > 65536, "the large launch must take the throughput family's big-job branch"
    chunk = 512 // tiles
    assert chunk >= 1
    w = model._cache.get("ins_seg", model.ins_seg, hip.HEAD_INS_SEG)
    x = pts.transpose(2, 1)
    g, lg, mk = _forward(w, c_in, x)
    for lo in range(0, B, chunk):
        hi = min(B, lo + chunk)
        g2, lg2, mk2 = _forward(w, c_in, x[lo:hi])
        same = _same_bits(g2, g[lo:hi])
        if not same:
            diff = (g2.view(torch.int32) != g[lo:hi].view(torch.int32))
            rows = torch.nonzero(diff.any(1)).flatten()[:8].tolist()
            worst = float((g2 - g[lo:hi]).abs().nan_to_num().max())
            print(f"{what}: rows {[lo + r for r in rows]} differ, {int(diff.sum())} entries, max |diff| {worst:g}")
        assert same, (what, lo)
        assert _same_bits(lg2, lg[lo:hi]) and torch.equal(mk2, mk[lo:hi]), (what, lo)
    return g


def test_c2_full_launch_equals_the_dense_family_on_every_row():
    """bench.py's flagship: StaticModelOneBoxEst's weights, 4096 crops x 1024 points"""
    pts_np, _, _ = synth.static_crops(4096, 1024)
    model = build_model("static_one", synth.state_dict("static_one"))
    g = _check(model, torch.from_numpy(pts_np).cuda(), 3, "C2")
    assert bool(torch.isfinite(g).all()) and float(g.max()) > 0


def test_dynamic_fp32_full_launch_equals_the_dense_family_on_every_row():
    """DynamicModel's segmentation net: c_in = 4, 1024 items x 5120 points (3 items per latency launch)"""
    p, _, _, _ = synth.dynamic_items(1024)
    model = build_model("dynamic", synth.state_dict("dynamic"))
    _check(model, torch.from_numpy(p).cuda(), 4, "Dynamic_fp32")


@pytest.mark.parametrize("B,N", [(300, 1000), (131, 1023), (1200, 77), (90, 4097)])
def test_ragged_point_counts(B, N):
    """N not a multiple of 32 / 64 / 256: the last wave's tiles replicate the crop's last point"""
    pts_np, _, _ = synth.static_crops(B, N, seed=N)
    model = build_model("static_one", synth.state_dict("static_one", seed=7))
    _check(model, torch.from_numpy(pts_np).cuda(), 3, f"ragged {B}x{N}")


def _adversarial(pts_np):
    p = pts_np.copy()
    N = p.shape[1]
    p[3, N // 2:] = p[3, :N // 2]                          # every point twice: exact ties in every channel
    p[5, :] = p[5, 0]                                       # all points equal: every point is an arg-max
    p[6, :] = 0.0
    p[9] *= np.float32(1e4)                                 # activations beyond fp16's range
    p[10, ::3] *= np.float32(1e4)                           # ... in some of the crop's tiles only
    p[12] *= np.float32(1e-6)                               # inputs below fp16's normal range
    p[13, 5:] = p[13, 4]                                    # five distinct points
    p[17, 100:164] *= np.float32(300.0)                     # one wave's points far from the others
    p[20] *= np.float32(40.0)
    return p


@pytest.mark.parametrize("scale5,shift5", [(1.0, 0.0), (1e3, 0.0), (1e-3, 0.0), (1.0, -50.0), (1e7, 0.0)])
def test_adversarial_crops_inside_a_large_batch(scale5, shift5):
    """duplicated points, constant crops, coordinates of 1e4 and 1e-6 placed in a batch of ordinary crops; conv5's weights
    scaled by 1e3 / 1e-3 / beyond fp16's range (the blob's flag: dense kernel), and a bias that makes the maximum of
    half of the channels negative (pooled value +0: no point may be a candidate there)"""
    B, N = 96, 1024
    pts_np, _, _ = synth.static_crops(B, N, seed=91)
    sd = dict(synth.state_dict("static_one", seed=91))
    sd["ins_seg.conv5.weight"] = (np.asarray(sd["ins_seg.conv5.weight"]) * np.float32(scale5)).astype(np.float32)
    if shift5:
        bias = np.asarray(sd["ins_seg.bn5.bias"]).astype(np.float32).copy()
        bias[::2] += np.float32(shift5)
        sd["ins_seg.bn5.bias"] = bias
    model = build_model("static_one", sd)
    g = _check(model, torch.from_numpy(_adversarial(pts_np)).cuda(), 3, f"adversarial x{scale5:g} {shift5:+g}")
    if shift5:
        assert float((g[:, ::2] == 0).float().mean()) > 0.9


def test_non_finite_crops_inside_a_large_batch():
    """NaN / Inf coordinates: the crop's pooled feature is the quiet-NaN pattern in every channel, as from the dense
    kernels; its neighbours are untouched"""
    B, N = 80, 1024
    pts_np, _, _ = synth.static_crops(B, N, seed=92)
    p = pts_np.copy()
    p[1, 7, 0] = np.nan
    p[3, 0, 2] = np.inf
    p[4, N - 1, 1] = -np.inf
    p[79, 500, 1] = np.nan
    model = build_model("static_one", synth.state_dict("static_one", seed=92))
    g = _check(model, torch.from_numpy(p).cuda(), 3, "non-finite")
    bad = [1, 3, 4, 79]
    good = [b for b in range(B) if b not in bad]
    assert bool(torch.isnan(g[bad]).all()) and bool(torch.isfinite(g[good]).all())
    clean = _check(model, torch.from_numpy(pts_np).cuda(), 3, "clean")
    assert torch.equal(clean[good], g[good])
