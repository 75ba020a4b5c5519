"""The fp32 throughput decoder as a pair of waves per tile (csrc/dal3_pointmlp.hip: ins_seg_decode_pair_kernel, DESIGN.md "Two
waves per tile"; the schedule's CPU model is tests/dec_pair_model.py) gives the BITS of the kernel with one wave per tile.

Every case is one `dal3_ins_seg_forward` on the throughput family (DAL3_BCN_NO_SMALL_JOB_KERNELS) against the same call with
DAL3_BCN_NO_DEC_PAIR: `torch.equal` on the bit patterns of the logits and on the mask of every row, and the route query has
to name the two kernels. The live sets are +-1e6 shifts on dconv1's folded bias in chain order, so every tile of every crop
has exactly that set: 3 crops x 1024 points, 3 x 1000 (a ragged last tile) and 2 x 96 (three pairs per crop: fewer than a
CU holds). A crop has a plan only where the screened encoder runs, above 65,536 points and 512 tiles: the plan cases take
tests/test_gpu_dec_prune.py's 520 crops x 128 points, the smallest batch with plans."""
import importlib

import numpy as np
import pytest
import torch

import dec_prune_model as P
from _common import build_model, synth
from dec_group_model import live_sets
from dec_queue_model import chain
from test_gpu_dec_prune import _plan, _planted
from test_gpu_dec_sparse import _blob, _guard_flag

hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu

THROUGHPUT = hip.BCN_NO_SMALL_JOB_KERNELS
SHAPES = [(3, 1024), (3, 1000), (2, 96)]
SETS = dict(live_sets(4))
SETS["odd totals in consecutive groups"] = np.zeros(512, bool)   # totals 1, 3, 5, 2: a leftover is written in three groups running
SETS["odd totals in consecutive groups"][[5, 128 + 31, 128 + 32, 256, 256 + 63, 256 + 64, 256 + 127, 384 + 77]] = True
SETS["nothing dead"] = np.ones(512, bool)                        # the identity plan with every chunk fully live


def _forward(w, c_in, x, flags):
    lib = hip.lib()
    B, _, N = x.shape
    ws = torch.zeros(lib.dal3_ins_seg_workspace_bytes(B), dtype=torch.uint8, device="cuda")
    lg = torch.empty((B, N, 2), device="cuda")
    mk = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    v = hip.bcn(x)
    v.flags |= flags
    hip.check(lib.dal3_ins_seg_forward(hip.ptr(w), hip.F32, c_in, v, B, N, hip.ptr(lg), hip.ptr(mk), None, hip.ptr(ws), ws.numel(),
                                       hip.stream()))
    return lg, mk, ws


def _pair_equals_one_wave(model, pts, c_in, what, guarded=False, flags=THROUGHPUT):
    """pts (B, N, c_in) on the GPU"""
    w = _blob(model)
    B, N, _ = pts.shape
    lib = hip.lib()
    assert _guard_flag(w) == int(guarded), what
    assert lib.dal3_ins_seg_decode_route(hip.ptr(w), B, N, flags | hip.BCN_NO_DEC_PAIR) == hip.DEC_ROUTE_ONE_WAVE, what
    assert lib.dal3_ins_seg_decode_route(hip.ptr(w), B, N, flags) == (hip.DEC_ROUTE_ONE_WAVE if guarded else hip.DEC_ROUTE_PAIR), what
    x = pts.transpose(2, 1)
    lg, mk, ws = _forward(w, c_in, x, flags)
    lg0, mk0, _ = _forward(w, c_in, x, flags | hip.BCN_NO_DEC_PAIR)
    same = torch.equal(lg.view(torch.int32), lg0.view(torch.int32))
    if not same:
        diff = (lg.view(torch.int32) != lg0.view(torch.int32)).any(2)
        print(f"{what}: crops {torch.nonzero(diff.any(1)).flatten()[:8].tolist()} differ, {int(diff.sum())} points, "
              f"first points {torch.nonzero(diff)[:4].tolist()}")
    assert same and torch.equal(mk, mk0), what
    return lg, mk, ws


def _shifted(seed, live=None, dead3=None, dead4=None, kind="static_one"):
    """synth weights; live (512,) bool in chain order: dconv1's term +1e6 on these, -1e6 on the others. dead3 (256,) / dead4
    (128,) bool in chain order: dconv2's / dconv3's folded bias far below what the live inputs can add, far above on the
    others, so that dconv3 / dconv4 see exactly that live set in every tile"""
    sd = dict(synth.state_dict(kind, seed=seed))

    def shift(key, dead, ch, size):
        s = np.where(dead, -size, size)
        out = np.asarray(sd[key]).astype(np.float32).copy()
        out[ch] += s.astype(np.float32)
        sd[key] = out

    if live is not None:
        shift("ins_seg.dbn1.bias", ~live, chain(512), 1e6)
    if dead3 is not None:
        shift("ins_seg.dbn2.bias", dead3, chain(256), 1e12)
    if dead4 is not None:
        shift("ins_seg.dbn3.bias", dead4, chain(128), 1e20)
    return sd


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["nothing live", "only 0", "nothing dead", "odd totals in consecutive groups",
                                  "leftover across dead groups", "odd per group", "random 0.45"])
def test_planted_live_sets(name, shape):
    """all 512 channels dead; one live; nothing dead; odd totals in consecutive groups (a leftover crosses two seams); a group
    entirely dead between two live ones; an odd count in every group; a random set"""
    B, N = shape
    model = build_model("static_one", _shifted(61, live=SETS[name]))
    pts = synth.static_crops(B, N, seed=61)[0]
    lg, _, _ = _pair_equals_one_wave(model, torch.from_numpy(pts).cuda(), 3, f"{name} {B}x{N}")
    assert bool(torch.isfinite(lg).all())


@pytest.mark.parametrize("n3,n4", [(155, 77), (1, 1), (256, 127)])
def test_odd_totals_in_dconv3_and_dconv4(n3, n4):
    """n3 of dconv3's 256 inputs and n4 of dconv4's 128 are live in every tile: the last k-step pairs a row with the zeros"""
    rng = np.random.default_rng(n3)
    dead3, dead4 = np.ones(256, bool), np.ones(128, bool)
    dead3[rng.permutation(256)[:n3]] = False
    dead4[rng.permutation(128)[:n4]] = False
    model = build_model("static_one", _shifted(62, live=SETS["random 0.45"], dead3=dead3, dead4=dead4))
    pts = synth.static_crops(3, 1000, seed=62)[0]
    lg, _, _ = _pair_equals_one_wave(model, torch.from_numpy(pts).cuda(), 3, f"dconv3 {n3} live, dconv4 {n4} live")
    assert bool(torch.isfinite(lg).all())


def test_synth_weights_as_they_are_and_four_input_channels():
    for kind, c_in, pts in (("static_one", 3, synth.static_crops(3, 1000, seed=63)[0]),
                            ("dynamic", 4, synth.dynamic_items(2, n_per_frame=100, seed=63)[0])):
        model = build_model(kind, synth.state_dict(kind, seed=63))
        _pair_equals_one_wave(model, torch.from_numpy(pts).cuda(), c_in, kind)


def test_plans_of_every_length():
    """520 crops x 128 points with 0 .. 512 live channels side by side (tests/test_gpu_dec_prune.py): plans of 2 chunks (the
    shortest last group), of 10 and 14 (a last group of two chunks behind full ones, in either buffer), of 4, and crops
    without a plan, which run the identity plan"""
    sd, pts_np, live = _planted(21)
    model = build_model("static_one", sd)
    lg, mk, ws = _pair_equals_one_wave(model, torch.from_numpy(pts_np).cuda(), 3, "plans", flags=0)
    nch = _plan(ws, 520)[4]
    assert set(nch.tolist()) >= {0, 2, 4, 10, 14}
    assert bool(torch.isfinite(lg).all())


def test_a_crop_with_a_non_finite_coordinate_beside_healthy_ones():
    pts = synth.static_crops(3, 1024, seed=64)[0].copy()
    pts[1, 700, 1] = np.nan
    model = build_model("static_one", _shifted(64, live=SETS["random 0.45"]))
    lg, mk, _ = _pair_equals_one_wave(model, torch.from_numpy(pts).cuda(), 3, "NaN crop")
    assert bool(torch.isnan(lg[1]).all()) and int(mk[1].sum()) == 0 and bool(torch.isfinite(lg[[0, 2]]).all())


@pytest.mark.parametrize("layer,rows", [("dconv2", 512), ("dconv3", 256), ("dconv4", 128), ("-0 bias", 0)])
def test_a_guarded_blob_runs_the_kernel_with_one_wave_per_tile(layer, rows):
    """an Inf weight in dconv2, dconv3 or dconv4, or a folded dconv2 bias of -0, sets the blob's guard flag: the route query
    names the old kernel, and the outputs are its outputs (the Inf weight sits on an input that is dead in every tile: a
    kernel that skipped the row would lose the NaN of 0 * Inf)"""
    live = SETS["random 0.45"]
    sd = _shifted(65, live=live)
    if rows:
        wt = np.asarray(sd[f"ins_seg.{layer}.weight"]).astype(np.float32).copy()
        col = int(chain(512)[np.nonzero(~live)[0][0]]) if rows == 512 else 3
        wt[3, col, 0] = np.inf
        sd[f"ins_seg.{layer}.weight"] = wt
    else:
        gamma = np.asarray(sd["ins_seg.dbn2.weight"]).astype(np.float32).copy()
        beta = np.asarray(sd["ins_seg.dbn2.bias"]).astype(np.float32).copy()
        bias = np.asarray(sd["ins_seg.dconv2.bias"]).astype(np.float32).copy()
        gamma[5] = -abs(gamma[5]) - np.float32(0.1)        # (b - mean) * s + beta = (+0) * (negative) + (-0) = -0
        beta[5] = np.float32(-0.0)
        bias[5] = np.asarray(sd["ins_seg.dbn2.running_mean"])[5]
        sd["ins_seg.dbn2.weight"], sd["ins_seg.dbn2.bias"], sd["ins_seg.dconv2.bias"] = gamma, beta, bias
    model = build_model("static_one", sd)
    pts = synth.static_crops(3, 1000, seed=65)[0]
    _pair_equals_one_wave(model, torch.from_numpy(pts).cuda(), 3, f"guard: {layer}", guarded=True)


def test_a_shard_with_an_item_offset():
    """the whole model on a shard (item_offset 5): every output tensor with the pairs and without them"""
    p, i, g = synth.static_crops(3, 1000, seed=66)
    got = {}
    for flags in (THROUGHPUT, THROUGHPUT | hip.BCN_NO_DEC_PAIR):
        model = build_model("static_one", synth.state_dict("static_one", seed=66))
        model.item_offset = 5
        hip.DISPATCH_FLAGS = flags
        try:
            o = model._run(torch.from_numpy(p).cuda().transpose(2, 1), torch.from_numpy(i).cuda(), torch.from_numpy(g).cuda())
        finally:
            hip.DISPATCH_FLAGS = 0
        got[flags] = {k: v.cpu().numpy() for k, v in o.items() if torch.is_tensor(v)}
    a, b = got[THROUGHPUT], got[THROUGHPUT | hip.BCN_NO_DEC_PAIR]
    assert set(a) == set(b) and "logits" in a and "mask" in a
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_the_route_query():
    lib = hip.lib()
    assert lib.dal3_ins_seg_decode_route(None, 4096, 1024, 0) == hip.DEC_ROUTE_PAIR
    assert lib.dal3_ins_seg_decode_route(None, 4096, 1024, hip.BCN_NO_DEC_PAIR) == hip.DEC_ROUTE_ONE_WAVE
    assert lib.dal3_ins_seg_decode_route(None, 16, 1024, 0) == hip.DEC_ROUTE_LATENCY          # 512 tiles: the small-job family
    assert lib.dal3_ins_seg_decode_route(None, 16, 1024, hip.BCN_NO_DEC_PAIR) == hip.DEC_ROUTE_LATENCY
    assert lib.dal3_ins_seg_decode_route(None, 16, 1024, THROUGHPUT) == hip.DEC_ROUTE_PAIR
    assert lib.dal3_ins_seg_decode_route(None, 4096, 1024, 256) < 0 and lib.dal3_ins_seg_decode_route(None, 0, 1024, 0) < 0
