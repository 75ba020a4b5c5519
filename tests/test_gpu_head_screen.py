"""The screened fp32 point heads (csrc/dal3_head_screen.hip) give the dense head's BITS.

The reference inside the library is `dal3_point_head_pool` WITHOUT a workspace: one dense workgroup per (item, tile),
which the screen does not touch. Every case runs the same batch with a workspace (the seed launch and the screened
launch) and asserts equality of the bit patterns of the pooled feature on ALL rows. The shapes are the smallest that
take the screen: just above the dispatch minimum the library reports. tests/test_head_screen_model.py holds the
condition that these inputs do go through the screen instead of its dense fall-backs."""
import importlib

import numpy as np
import pytest
import torch

import head_screen_model as H
from _common import build_model, recentred_sd, synth

hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu

HEADS = [("static_one", "box_est", 3, 512), ("dynamic", "point_emb", 4, 2560)]


def _pool(mod, w, x, distinct, ws):
    """x (B,M,c) on the GPU -> feat (B,512); ws None: the per-tile dense launch"""
    lib = hip.lib()
    B, M, _ = x.shape
    f = torch.empty((B, 512), device="cuda")
    hip.check(lib.dal3_point_head_pool(mod.HEAD_KIND, hip.ptr(w), hip.F32, hip.bcn(x.transpose(2, 1)), B, M, hip.ptr(distinct),
                                       hip.ptr(f), hip.ptr(ws), ws.numel() if ws is not None else 0, hip.stream()))
    return f


def _check(kind, head, sd, x_np, d_np, what):
    lib = hip.lib()
    B, M, _ = x_np.shape
    assert B * ((M + 31) // 32) >= lib.dal3_point_head_screen_min_tiles(), "the launch must take the screened route"
    model = build_model(kind, sd)
    mod = getattr(model, head)
    w = model._cache.get(head, mod, mod.HEAD_KIND, hip.F32)
    x = torch.from_numpy(x_np).cuda()
    ws = torch.empty(int(lib.dal3_point_head_pool_workspace_bytes(B, M)), dtype=torch.uint8, device="cuda")
    out = None
    for distinct in ((torch.from_numpy(d_np).cuda(), None) if d_np is not None else (None,)):
        got, want = _pool(mod, w, x, distinct, ws), _pool(mod, w, x, distinct, None)
        torch.cuda.synchronize()
        diff = got.view(torch.int32) != want.view(torch.int32)
        if bool(diff.any()):
            rows = torch.nonzero(diff.any(1)).flatten()[:8].tolist()
            print(f"{what}: rows {rows} differ, {int(diff.sum())} entries, max |diff| {float((got - want).abs().nan_to_num().max()):g}")
        assert not bool(diff.any()), what
        out = got if out is None else out
    return out


@pytest.mark.parametrize("kind,head,c_in,M", HEADS)
def test_every_row_equals_the_per_tile_dense_launch(kind, head, c_in, M):
    """kind 1 at B x 512 and kind 2 at B x 2560, B just above the dispatch minimum; counts of distinct points 0, 1, 31, 32,
    33, 32 S - 1, 32 S, 32 S + 1, M - 1, M in front of random ones, and no counts at all: items with seed tiles only, with
    exactly one screened tile, with ragged last tiles"""
    B = H.gpu_batch(M)
    sd, x, d = H.gpu_case(kind, head, c_in, B, M, stride=hip.lib().dal3_point_head_screen_stride())
    f = _check(kind, head, sd, x, d, f"{head} {B}x{M}")
    assert bool(torch.isfinite(f).all()) and float(f.max()) > 0


def _adversarial_batch(scale4=1.0, shift4=0.0, tiny_rows=False):
    M = 512
    B = H.gpu_batch(M)
    sd, x, d = H.gpu_case("static_one", "box_est", 3, B, M)
    sd = dict(sd)
    n0 = len(H.special_counts(M))
    o, dd = H.adversarial(torch.from_numpy(x[n0:n0 + 8]), d[n0:n0 + 8])
    x[n0:n0 + 8], d[n0:n0 + 8] = o.numpy(), dd
    w = np.asarray(sd["box_est.conv4.weight"]).astype(np.float32) * np.float32(scale4)
    if tiny_rows:
        w[::4] = w[::4] * np.float32(2.0 ** -130)
    sd["box_est.conv4.weight"] = w
    if shift4:
        bias = np.asarray(sd["box_est.bn4.bias"]).astype(np.float32).copy()
        bias[::2] += np.float32(shift4)
        sd["box_est.bn4.bias"] = bias
    return sd, x, d


@pytest.mark.parametrize("scale4,shift4", [(1.0, 0.0), (1e3, 0.0), (1e-3, 0.0), (1.0, -50.0), (1e7, 0.0)])
def test_adversarial_items_inside_a_batch_of_ordinary_ones(scale4, shift4):
    """duplicated points, all points equal, one live point, coordinates x 1e4 (beyond fp16: dense tiles) and x 1e-6; conv4
    scaled by 1e3 / 1e-3 / beyond fp16's range (the blob's flag: every tile dense), and a bias that makes half of the
    maxima negative (pooled value +0)"""
    sd, x, d = _adversarial_batch(scale4, shift4)
    f = _check("static_one", "box_est", sd, x, d, f"adversarial x{scale4:g} {shift4:+g}")
    if shift4:
        assert float((f[:, ::2] == 0).float().mean()) > 0.9


def test_more_candidates_than_the_list_holds_and_subnormal_sums():
    """every fourth conv4 row scaled by 2^-130: its scores are 0 in fp16 and its threshold lies within E of them, so every
    point of the tile is a candidate in 128 channels (4096 > the list's 1024: the dense layer), and the rows' chains sum
    subnormals, on the MFMA in one launch and in the other"""
    sd, x, d = _adversarial_batch(tiny_rows=True)
    _check("static_one", "box_est", sd, x, d, "tiny rows")


def test_a_non_finite_item_keeps_its_nan_row():
    sd, x, d = _adversarial_batch()
    x[40, 7, 0] = np.nan
    x[41, 300, 2] = np.inf
    d[40] = d[41] = 512
    f = _check("static_one", "box_est", sd, x, d, "non-finite")
    bad = [40, 41]
    good = [b for b in range(x.shape[0]) if b not in bad]
    assert bool(torch.isnan(f[bad]).all()) and bool(torch.isfinite(f[good]).all())
    assert bool((f[bad].view(torch.int32) == 0x7FC00000).all())


def test_refine_equals_the_run_without_the_worklist():
    """end to end: model.refine on bench crops (300, or as many as the dispatch minimum asks for) gives the same boxes with
    the screened head as with DAL3_BCN_NO_WORKLIST (the per-tile dense launch)"""
    n = max(300, H.gpu_batch(512))
    pts_np, init_np, _ = synth.static_crops(n, 1024)
    model = build_model("static_one", recentred_sd("static_one", pts_np[:32], synth.SEED))
    pts, init = torch.from_numpy(pts_np).cuda().transpose(2, 1), torch.from_numpy(init_np).cuda()
    a = model.refine(pts, init).clone()
    hip.DISPATCH_FLAGS = hip.BCN_NO_WORKLIST
    try:
        b = model.refine(pts, init).clone()
    finally:
        hip.DISPATCH_FLAGS = 0
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bool(torch.isfinite(a).all())
