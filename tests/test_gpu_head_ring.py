"""The fp16 weight ring of the screened point heads (csrc/dal3_head_screen.hip) stands at the stream's start at every tile
boundary, whichever way the tile before went.

A persistent wave of the screened launch takes tile after tile; its ring of conv4's fp16 fragments is read at offsets that
are a function of the sweep's own counters, and a tile that leaves the screen (range, the blob's flag, list overflow)
must hand the ring on exactly as a screened one does. The job is the smallest that takes the screened route, 512 items of
512 points = 8192 tiles; the reference is the DENSE persistent route of the same library, which the same items take in two
halves of 4096 tiles (below the dispatch minimum), and every row's bit patterns are compared. One batch holds, in worklist
order: items of two tiles (one screened tile each, so that a wave's run crosses from item to item), ragged last tiles, an
item whose tile 2 has coordinates of 1e4 between its screened tiles 1 and 3, an item of 512 equal points (every pair a
candidate: the list overflows), two items with a non-finite point, then ordinary items. A second batch has conv4 scaled
beyond fp16's range: the blob's flag, every tile dense. tests/head_screen_model.py tells that the two special items do
leave the screen the intended way."""
import functools
import importlib

import numpy as np
import pytest
import torch

import head_screen_model as H
from _common import build_model, synth

hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu

B, M = 512, 512
HEADS = [("static_one", "box_est", 3), ("dynamic", "point_emb", 4)]
TWO_TILES = range(0, 8)
RAGGED2, RAGGED6, RANGE, EQUAL, NAN, INF, ORDINARY = 8, 9, 10, 11, 12, 13, 14


def _batch(kind, c_in):
    """(x (B,M,c_in) fp32, distinct (B,) int32), the caller's own copies"""
    x, d = _batch_once(kind, c_in)
    return x.copy(), d.copy()


@functools.lru_cache(maxsize=None)
def _batch_once(kind, c_in):
    rng = np.random.default_rng(17)
    if kind == "static_one":
        pts = synth.static_crops(B, M, seed=5)[0]
    else:
        pts = synth.dynamic_items(B, n_per_frame=128, seed=5)[0][:, :M]
    x = np.ascontiguousarray(pts[:, :, :c_in]).astype(np.float32)
    d = np.full(B, M, np.int32)
    d[ORDINARY::4] = rng.integers(1, M + 1, size=len(d[ORDINARY::4]))
    d[list(TWO_TILES)] = 64
    d[RAGGED2], d[RAGGED6] = 40, 32 * 5 + 7
    for b in range(B):                                    # beyond an item's count: copies of its first points
        k = int(d[b])
        x[b, k:] = x[b, np.arange(M - k) % k]
    x[RANGE, 64:96] *= np.float32(1e4)
    x[EQUAL, :] = x[EQUAL, 0]
    return x, d


def _pool(mod, w, x, distinct, ws):
    lib = hip.lib()
    n = x.shape[0]
    f = torch.empty((n, 512), device="cuda")
    hip.check(lib.dal3_point_head_pool(mod.HEAD_KIND, hip.ptr(w), hip.F32, hip.bcn(x.transpose(2, 1)), n, M, hip.ptr(distinct),
                                       hip.ptr(f), hip.ptr(ws), ws.numel(), hip.stream()))
    return f


def _screened_and_dense(kind, head, sd, x_np, d_np):
    """(the screened route's feat, the dense persistent route's feat) of the batch, both (B,512) on the GPU"""
    lib = hip.lib()
    tiles = (M + 31) // 32
    lo = int(lib.dal3_point_head_screen_min_tiles())
    assert B * tiles >= lo > (B // 2) * tiles, "the batch takes the screened route, each half of it the dense persistent one"
    model = build_model(kind, sd)
    mod = getattr(model, head)
    w = model._cache.get(head, mod, mod.HEAD_KIND, hip.F32)
    x, d = torch.from_numpy(x_np).cuda(), torch.from_numpy(d_np).cuda()
    ws = torch.empty(int(lib.dal3_point_head_pool_workspace_bytes(B, M)), dtype=torch.uint8, device="cuda")
    got = _pool(mod, w, x, d, ws)
    h = B // 2
    want = torch.cat([_pool(mod, w, x[:h].contiguous(), d[:h].contiguous(), ws),
                      _pool(mod, w, x[h:].contiguous(), d[h:].contiguous(), ws)])
    torch.cuda.synchronize()
    return got, want


def _assert_same_bits(got, want, what):
    diff = got.view(torch.int32) != want.view(torch.int32)
    if bool(diff.any()):
        rows = torch.nonzero(diff.any(1)).flatten()[:8].tolist()
        print(f"{what}: rows {rows} differ, {int(diff.sum())} entries, max |diff| {float((got - want).abs().nan_to_num().max()):g}")
    assert not bool(diff.any()), what


@pytest.mark.parametrize("kind,head,c_in", HEADS)
def test_every_way_through_a_tile_leaves_the_ring_at_the_streams_start(kind, head, c_in):
    sd = synth.state_dict(kind, seed=23)
    x, d = _batch(kind, c_in)
    # the two special items do leave the screen: tile 2 for range, the equal points for the list's capacity
    r = H.run(sd, x[[RANGE]], d[[RANGE]], p=head, proof=False)
    assert r["tiles_dense_for_range"] == 1 and r["screened_tiles"] == 11, r
    r = H.run(sd, x[[EQUAL]], d[[EQUAL]], p=head, proof=False)
    assert r["tiles_dense_for_range"] == 0 and r["tiles_over_cap"] > 0, r
    x[NAN, 7, 0] = np.nan
    x[INF, 300, 2] = np.inf
    got, want = _screened_and_dense(kind, head, sd, x, d)
    _assert_same_bits(got, want, f"{head} {B}x{M}")
    bad = [NAN, INF]
    good = [b for b in range(B) if b not in bad]
    assert bool((got[bad].view(torch.int32) == 0x7FC00000).all()) and bool(torch.isfinite(got[good]).all())
    assert float(got[good].max()) > 0


@pytest.mark.parametrize("kind,head,c_in", HEADS)
def test_the_blob_flag_route(kind, head, c_in):
    """conv4 beyond fp16's range: every tile of the screened launch takes the dense layer and no sweep ever runs"""
    sd = dict(synth.state_dict(kind, seed=23))
    sd[f"{head}.conv4.weight"] = np.asarray(sd[f"{head}.conv4.weight"]).astype(np.float32) * np.float32(1e7)
    x, d = _batch(kind, c_in)
    got, want = _screened_and_dense(kind, head, sd, x, d)
    _assert_same_bits(got, want, f"{head} {B}x{M}, conv4 x 1e7")
    assert float(got.nan_to_num().max()) > 0
