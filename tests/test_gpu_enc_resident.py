"""The crop-resident screened encoder (csrc/dal3_enc_screen.hip, ins_seg_encode_resident_kernel) gives the BITS of the
screened encoder's two launches and of the dense latency family.

Every case runs one `dal3_ins_seg_forward` launch of the smallest batch that the route rule sends to the resident
kernel (asserted through `dal3_ins_seg_encoder_route`) and compares, on ALL rows and as bit patterns with no tolerance,
  - the pooled feature g, the decoder plan's `prune` rows (dal3_ins_seg_plan_layout), the logits and the mask with the
    same launch under DAL3_BCN_NO_ENC_RESIDENT (the two launches), and
  - g, the logits and the mask with the same crops in chunks small enough for the latency family.
The special crops are planted among ordinary ones, at the start and at the end of the batch."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

from _common import build_model, synth

hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu

SLOT = 64                                                  # 32 * DAL3_ENC_T points
FORTY = 7 + 25 * np.arange(40)


def _forward(w, c_in, x, flags=0):
    """x: (B, c_in, N) view on the GPU -> (g, logits, mask, prune rows (B,513) int32) of one dal3_ins_seg_forward launch"""
    lib = hip.lib()
    B, _, N = x.shape
    ws = torch.zeros(lib.dal3_ins_seg_workspace_bytes(B), dtype=torch.uint8, device="cuda")
    g = torch.empty((B, 1024), device="cuda")
    lg = torch.empty((B, N, 2), device="cuda")
    mk = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    v = hip.bcn(x)
    v.flags |= flags
    hip.check(lib.dal3_ins_seg_forward(hip.ptr(w), hip.F32, c_in, v, B, N, hip.ptr(lg), hip.ptr(mk), hip.ptr(g),
                                       hip.ptr(ws), ws.numel(), hip.stream()))
    off = (C.c_size_t * 4)()
    hip.check(lib.dal3_ins_seg_plan_layout(B, off, None))
    prune = ws[off[0]:off[0] + 4 * 513 * B].view(torch.int32).view(B, 513).clone()
    return g, lg, mk, prune


def _bits(t):
    return t.view(torch.int32)


@functools.lru_cache(maxsize=None)
def _smallest_resident_batch(N):
    """the smallest B whose (B, N) job takes the resident route (the rule is monotone in B)"""
    route = lambda B: hip.lib().dal3_ins_seg_encoder_route(B, N, 0)
    hi = 1
    while route(hi) != hip.ENC_ROUTE_RESIDENT:
        hi *= 2
        assert hi <= 1 << 16, "no batch takes the resident route"
    lo = hi // 2                                           # route(lo) is not resident (or lo == 0)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if route(mid) == hip.ENC_ROUTE_RESIDENT else (mid, hi)
    return hi


def _check(model, pts, c_in, what):
    """pts: (B, N, c_in) on the GPU"""
    lib = hip.lib()
    B, N, _ = pts.shape
    assert lib.dal3_ins_seg_encoder_route(B, N, 0) == hip.ENC_ROUTE_RESIDENT, what
    assert lib.dal3_ins_seg_encoder_route(B - 1, N, 0) != hip.ENC_ROUTE_RESIDENT, what
    assert lib.dal3_ins_seg_encoder_route(B, N, hip.BCN_NO_ENC_RESIDENT) == hip.ENC_ROUTE_TWO_LAUNCH, what
    w = model._cache.get("ins_seg", model.ins_seg, hip.HEAD_INS_SEG)
    x = pts.transpose(2, 1)
    g, lg, mk, prune = _forward(w, c_in, x)
    g2, lg2, mk2, prune2 = _forward(w, c_in, x, hip.BCN_NO_ENC_RESIDENT)
    same = torch.equal(_bits(g), _bits(g2))
    if not same:
        diff = _bits(g) != _bits(g2)
        print(f"{what}: rows {torch.nonzero(diff.any(1)).flatten()[:8].tolist()} differ from the two launches, {int(diff.sum())} "
              f"entries, max |diff| {float((g - g2).abs().nan_to_num().max()):g}")
    assert same, (what, "g against the two launches")
    assert torch.equal(prune, prune2), (what, "prune rows against the two launches")
    assert torch.equal(_bits(lg), _bits(lg2)) and torch.equal(mk, mk2), (what, "logits / mask against the two launches")
    tiles = (N + 31) // 32
    chunk = 512 // tiles
    assert chunk >= 1
    for lo in range(0, B, chunk):
        hi = min(B, lo + chunk)
        assert lib.dal3_ins_seg_encoder_route(hi - lo, N, 0) == hip.ENC_ROUTE_LATENCY
        g3, lg3, mk3, _ = _forward(w, c_in, x[lo:hi])
        assert torch.equal(_bits(g3), _bits(g[lo:hi])), (what, lo, "g against the latency family")
        assert torch.equal(_bits(lg3), _bits(lg[lo:hi])) and torch.equal(mk3, mk[lo:hi]), (what, lo, "logits / mask against the latency family")
    return g


def _plant(base, B):
    """(32, N, C) crops -> (B, N, C): the ordinary crops repeated, the special ones at rows 0.. and again at the end. Returns
    the batch and the row of the crop with a non-finite coordinate."""
    N = base.shape[1]
    slot = np.arange(N) // SLOT
    slots = -(-N // SLOT)
    R = -(-slots // 4)
    first = np.isin(slot, [R * w for w in range(4)])       # round 0's slots
    last = np.isin(slot, [R - 1 + R * w for w in range(4)])
    sp = base[:16].copy()
    sp[0, N // 2:2 * (N // 2)] = sp[0, :N // 2]             # every point twice: exact ties
    sp[1, :] = sp[1, 0]                                     # a constant crop
    sp[2, :] = 0.0
    sp[3, first] *= np.float32(1e4)                         # beyond fp16 in round 0's slots only: no bound at all
    sp[4, ~first] *= np.float32(1e4)                        # ... in the later slots only
    sp[5] *= np.float32(1e4)                                # ... in the whole crop
    sp[6, slot % 3 == 1] *= np.float32(1e4)                 # dense waves before, inside and after the screen
    sp[7] *= np.float32(1e-6)
    sp[8, first] = 0.0                                      # the bound is useless: round 0 at the origin,
    sp[8, ~first] *= np.float32(40.0)                       # the others far away
    sp[9, last] *= np.float32(25.0)                         # the crop's largest points in the last round only
    sp[10, N // 3, 0] = np.nan                              # a non-finite coordinate
    sp[11, 5:] = sp[11, 4]                                  # five distinct points
    p = np.concatenate([base] * (-(-B // base.shape[0])))[:B].copy()
    p[1:13] = sp[:12]
    p[B - 13:B - 1] = sp[:12][::-1]
    return p, [11, B - 2 - 10]


def _static(N, seed, sd=None):
    B = _smallest_resident_batch(N)
    model = build_model("static_one", sd if sd is not None else synth.state_dict("static_one", seed=seed))
    p, bad = _plant(synth.static_crops(32, N, seed=seed)[0], B)
    g = _check(model, torch.from_numpy(p).cuda(), 3, f"{B} x {N}")
    assert bool(torch.isnan(g[bad]).all()) and bool((_bits(g[bad]) == _bits(g[bad])[0, 0]).all()), "the NaN row stays"
    assert not bool(torch.isnan(g[20:40]).any())
    return g


@pytest.mark.parametrize("N", [64, 65, 255, 256, 257])
def test_short_crops_idle_waves_meet_the_barrier(N):
    """one to five slots: waves idle in round 0 (and in the only round), R = 1 and 2"""
    _static(N, seed=N)


@pytest.mark.parametrize("N", [1000, 1024, 1088])
def test_ragged_last_round(N):
    """R = 4 and 5; the last slot ragged, the last round not full"""
    _static(N, seed=N)


def test_long_crops_with_dynamic_weights():
    """N = 5120, c_in = 4: R = 20 rounds"""
    N = 5120
    B = _smallest_resident_batch(N)
    base = synth.dynamic_items(32)[0]
    assert base.shape[1:] == (N, 4)
    p, _ = _plant(base, B)
    _check(build_model("dynamic", synth.state_dict("dynamic")), torch.from_numpy(p).cuda(), 4, f"{B} x {N} dynamic")


@pytest.mark.parametrize("scale5,shift5", [(1e3, 0.0), (1e-3, 0.0), (1e7, 0.0), (1.0, -50.0)])
def test_conv5_scalings_and_negative_maxima(scale5, shift5):
    """conv5 x 1e3 / 1e-3; x 1e7 sets the blob's flag (no bound phase, every slot dense); a bias of -50 on every second
    channel: the pooled value is +0 there and no point may be a candidate"""
    sd = dict(synth.state_dict("static_one", seed=91))
    sd["ins_seg.conv5.weight"] = (np.asarray(sd["ins_seg.conv5.weight"]) * np.float32(scale5)).astype(np.float32)
    if shift5:
        bias = np.asarray(sd["ins_seg.bn5.bias"]).astype(np.float32).copy()
        bias[::2] += np.float32(shift5)
        sd["ins_seg.bn5.bias"] = bias
    g = _static(1024, seed=91, sd=sd)
    if shift5:
        assert float((g[20:40, ::2] == 0).float().mean()) > 0.9


def test_list_overflow_in_the_middle_of_a_crops_rounds():
    """40 conv5 rows scaled by 2^-130 (tests/test_gpu_tiny_magnitudes.py): every point is a candidate of those channels,
    1280 per tile exceed SCR_CAP, and the slot takes the dense layer while the crop's rounds go on"""
    sd = dict(synth.state_dict("static_one", seed=62))
    w = np.asarray(sd["ins_seg.conv5.weight"]).astype(np.float32).copy()
    w[FORTY] = w[FORTY] * np.float32(2.0 ** -130)
    sd["ins_seg.conv5.weight"] = w
    _static(1000, seed=62, sd=sd)
