"""The item-resident screened point head (csrc/dal3_head_screen.hip, point_head_resident_kernel) gives the dense head's BITS.

The batch is the smallest that `dal3_point_head_route` sends to the resident kernel (no constant is copied here). Every
row's bit patterns are compared with
    the DENSE persistent route of the same library, which the same items take in pieces of fewer tiles than the
    screen's dispatch minimum under DAL3_BCN_NO_HEAD_RESIDENT (asserted through the route function), and
    the same launch under DAL3_BCN_NO_HEAD_RESIDENT: the two launches, or at M = 160 the dense persistent kernel.
M = 160 is five tiles: the second round has one wave. The first rows hold the items that take another way through the
kernel: counts that the library clamps, one tile with three idle waves at the barrier, one full round, ragged tiles,
exact ties, 512 equal points (the list overflows in round 0: tests/head_resident_model.py confirms it), a tile at
coordinates of 1e4 in round 0 and one in a later round (dense for range; the first gives no bound), a NaN and an Inf
item. A second batch has conv4 beyond fp16's range: the blob's flag, every tile dense."""
import functools
import importlib

import numpy as np
import pytest
import torch

import head_resident_model as RM
from _common import build_model, synth

hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu

HEADS = {"box_est": ("static_one", 3), "point_emb": ("dynamic", 4)}
KIND = {"box_est": hip.HEAD_STATIC_BOX_EST, "point_emb": hip.HEAD_POINT_EMB}
TIES, EQUAL, RANGE0, RANGE1, NAN, INF = 10, 11, 12, 13, 14, 15


def _counts(M):
    """distinct <= 0 and > M, then 1, 31, 32, 33, 128, 129 and M - 1: items 0 .. 9"""
    return [0, -3, M + 5, 1, 31, 32, 33, 128, 129, M - 1]


@functools.lru_cache(maxsize=None)
def _resident_batch(head, M):
    """the smallest B that the library sends to the resident kernel at M points, by bisection on the route function"""
    lib = hip.lib()
    hk = KIND[head]
    route = lambda B, flags=0: lib.dal3_point_head_route(hk, B, M, flags)
    hi = 1
    while route(hi) != hip.HEAD_ROUTE_RESIDENT:
        hi *= 2
        assert hi <= 1 << 16, "no batch takes the resident route"
    lo = hi // 2                                           # route(lo) is not resident (or lo == 0)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if route(mid) == hip.HEAD_ROUTE_RESIDENT else (mid, hi)
    assert route(hi) == hip.HEAD_ROUTE_RESIDENT and route(hi - 1) != hip.HEAD_ROUTE_RESIDENT
    assert route(hi, hip.BCN_NO_HEAD_RESIDENT) in (hip.HEAD_ROUTE_TWO_LAUNCH, hip.HEAD_ROUTE_PERSISTENT)
    return hi


@functools.lru_cache(maxsize=None)
def _points(kind, c_in, B):
    if kind == "static_one":
        pts = synth.static_crops(B, 512, seed=5)[0]
    else:
        pts = synth.dynamic_items(B, n_per_frame=128, seed=5)[0][:, :512]
    return np.ascontiguousarray(pts[:, :, :c_in]).astype(np.float32)


def _batch(head, M):
    """(x (B,M,c_in) fp32, distinct (B,) int32) with the special items in front"""
    kind, c_in = HEADS[head]
    B = _resident_batch(head, M)
    rng = np.random.default_rng(17 + M)
    x = _points(kind, c_in, B)[:, :M].copy()
    d = rng.integers(1, M + 1, size=B).astype(np.int32)
    d[::3] = M
    sp = _counts(M)
    d[:len(sp)] = sp
    d[[TIES, EQUAL, RANGE0, RANGE1, NAN, INF]] = M
    for b in range(B):                                     # beyond an item's count: copies of its first points
        k = int(min(max(d[b], 1), M))
        x[b, k:] = x[b, np.arange(M - k) % k]
    x[TIES, M // 2:] = x[TIES, :M - M // 2]                # duplicated points: exact ties
    x[EQUAL, :] = x[EQUAL, 0]
    x[RANGE0, 0:32] *= np.float32(1e4)                     # tile 0: round 0
    x[RANGE1, 32:64] *= np.float32(1e4)                    # tile 1: round 1 (five tiles or more: two rounds at least)
    return x, d


def _pool(mod, w, x, distinct, ws, flags=0):
    lib = hip.lib()
    n, M, _ = x.shape
    f = torch.empty((n, 512), device="cuda")
    v = hip.bcn(x.transpose(2, 1))
    v.flags |= flags
    hip.check(lib.dal3_point_head_pool(mod.HEAD_KIND, hip.ptr(w), hip.F32, v, n, M, hip.ptr(distinct), hip.ptr(f), hip.ptr(ws),
                                       ws.numel(), hip.stream()))
    return f


def _three_routes(head, sd, x_np, d_np):
    """(resident, the same launch under the flag, the dense persistent route in pieces), each (B,512) on the GPU"""
    lib = hip.lib()
    kind, _ = HEADS[head]
    B, M, _ = x_np.shape
    tiles = (M + 31) // 32
    model = build_model(kind, sd)
    mod = getattr(model, head)
    w = model._cache.get(head, mod, mod.HEAD_KIND, hip.F32)
    x, d = torch.from_numpy(x_np).cuda(), torch.from_numpy(d_np).cuda()
    ws = torch.empty(int(lib.dal3_point_head_pool_workspace_bytes(B, M)), dtype=torch.uint8, device="cuda")
    assert lib.dal3_point_head_route(mod.HEAD_KIND, B, M, 0) == hip.HEAD_ROUTE_RESIDENT
    got = _pool(mod, w, x, d, ws)
    flagged = _pool(mod, w, x, d, ws, hip.BCN_NO_HEAD_RESIDENT)
    pieces = -(-B * tiles // (int(lib.dal3_point_head_screen_min_tiles()) - 1))
    edges = [B * i // pieces for i in range(pieces + 1)]
    dense = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        assert lib.dal3_point_head_route(mod.HEAD_KIND, hi - lo, M, hip.BCN_NO_HEAD_RESIDENT) == hip.HEAD_ROUTE_PERSISTENT
        dense.append(_pool(mod, w, x[lo:hi].contiguous(), d[lo:hi].contiguous(), ws, hip.BCN_NO_HEAD_RESIDENT))
    torch.cuda.synchronize()
    return got, flagged, torch.cat(dense)


def _assert_same_bits(got, want, what):
    diff = got.view(torch.int32) != want.view(torch.int32)
    if bool(diff.any()):
        rows = torch.nonzero(diff.any(1)).flatten()[:8].tolist()
        print(f"{what}: rows {rows} differ, {int(diff.sum())} entries, max |diff| {float((got - want).abs().nan_to_num().max()):g}")
    assert not bool(diff.any()), what


@pytest.mark.parametrize("M", [160, 512, 500])
@pytest.mark.parametrize("head", sorted(HEADS))
def test_every_row_equals_the_dense_route_and_the_two_launches(head, M):
    kind, _ = HEADS[head]
    sd = synth.state_dict(kind, seed=23)
    x, d = _batch(head, M)
    # the special items do go the intended way: the equal points overflow the list in round 0, the 1e4 tiles are dense
    # for range in round 0 and in round 1
    case = RM.Case(sd, x[[EQUAL, RANGE0, RANGE1]], d[[EQUAL, RANGE0, RANGE1]], p=head, what="special items")
    assert case.range_dense[1:].tolist() == [[t == 0 for t in range(case.nt)], [t == 1 for t in range(case.nt)]]
    assert RM.slot_map(case.nt)[1][0] == 1
    s16, E, b4 = case.s16[0], case.E[0], case.b4
    first = RM.slot_map(case.nt)[0]
    m = torch.stack([s16[:, 32 * t:32 * t + 32].amax(1) for t in first], 1)
    G0 = torch.relu(RM.bound_phase(m, E[:, first], b4[:, None]).amax(1))
    thr = (G0 - b4) - ((G0.abs() + b4.abs()) * 2.0 ** -22 + E[:, 0])
    assert int((s16[:, :32] > thr[:, None]).sum()) > 1024, "the equal points do not overflow the list in round 0"
    x[NAN, 7, 0] = np.nan
    x[INF, M - 20, 2] = np.inf
    got, flagged, dense = _three_routes(head, sd, x, d)
    _assert_same_bits(got, dense, f"{head} {x.shape[0]}x{M} against the dense persistent route")
    _assert_same_bits(got, flagged, f"{head} {x.shape[0]}x{M} against the same launch under DAL3_BCN_NO_HEAD_RESIDENT")
    bad = [NAN, INF]
    good = [b for b in range(x.shape[0]) if b not in bad]
    assert bool((got[bad].view(torch.int32) == 0x7FC00000).all()) and bool(torch.isfinite(got[good]).all())
    assert float(got[good].max()) > 0


@pytest.mark.parametrize("head", sorted(HEADS))
def test_the_blob_flag_route(head):
    """conv4 beyond fp16's range: every tile takes the dense layer after round 0's barrier and no sweep ever runs"""
    kind, _ = HEADS[head]
    sd = dict(synth.state_dict(kind, seed=23))
    sd[f"{head}.conv4.weight"] = np.asarray(sd[f"{head}.conv4.weight"]).astype(np.float32) * np.float32(1e7)
    x, d = _batch(head, 160)
    got, flagged, dense = _three_routes(head, sd, x, d)
    _assert_same_bits(got, dense, f"{head} {x.shape[0]}x160, conv4 x 1e7, against the dense persistent route")
    _assert_same_bits(got, flagged, f"{head} {x.shape[0]}x160, conv4 x 1e7, under DAL3_BCN_NO_HEAD_RESIDENT")
    assert float(got.nan_to_num().max()) > 0
