"""The compacted dconv2 of the fp32 throughput decoder (csrc/dal3_pointmlp.hip, DESIGN.md "Compacted dconv2") gives the
dense decoder's BITS.

The dense reference inside the library is the latency family (csrc/dal3_latency.hip), which `launch_ins_seg_decode`
takes for jobs of at most 512 tiles of 32 points and which the compaction does not touch. Every case pushes one large
launch (the throughput kernels) and the same crops in chunks small enough for the latency family through
`dal3_ins_seg_forward`, and asserts `torch.equal` on the logits and the mask of ALL rows — no sampling, no tolerance —
and on the pooled feature they start from (the pattern of tests/test_gpu_enc_screen.py)."""
import importlib

import numpy as np
import pytest
import torch

from _common import build_model, synth

hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu

BLOB_TAIL_BYTES = 32768                                    # DAL3_BLOB_TAIL_FLOATS * 4 (csrc/dal3_kernels.h)


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


def _blob(model):
    return model._cache.get("ins_seg", model.ins_seg, hip.HEAD_INS_SEG)


def _guard_flag(w):
    """the blob's dense-only flag: the last 256-byte section in front of the tail padding (csrc/dal3_api.hip, ins_seg_walk)"""
    at = w.numel() - BLOB_TAIL_BYTES - 256
    return int(w[at:at + 4].view(torch.int32).item())


def _check(model, pts, c_in, what):
    """pts: (B, N, c_in) on the GPU. One launch against chunks of at most 512 tiles."""
    B, N, _ = pts.shape
    tiles = (N + 31) // 32
    assert B * tiles > 512, "the large launch must take the throughput family"
    chunk = 512 // tiles
    assert chunk >= 1
    w = _blob(model)
    x = pts.transpose(2, 1)
    g, lg, mk = _forward(w, c_in, x)
    for lo in range(0, B, chunk):
        hi = min(B, lo + chunk)
        g2, lg2, mk2 = _forward(w, c_in, x[lo:hi])
        assert _same_bits(g2, g[lo:hi]), (what, lo)
        same = _same_bits(lg2, lg[lo:hi])
        if not same:
            diff = (lg2.view(torch.int32) != lg[lo:hi].view(torch.int32)).any(2)
            rows = torch.nonzero(diff.any(1)).flatten()[:8].tolist()
            worst = float((lg2 - lg[lo:hi]).abs().nan_to_num().max())
            print(f"{what}: crops {[lo + r for r in rows]} differ, {int(diff.sum())} points, max |diff| {worst:g}")
        assert same, (what, lo)
        assert torch.equal(mk2, mk[lo:hi]), (what, lo)
    return lg, mk


def test_c2_full_launch_equals_the_dense_family_on_every_row():
    """bench.py's flagship: StaticModelOneBoxEst's weights, 4096 crops x 1024 points"""
    pts_np, _, _ = synth.static_crops(4096, 1024)
    model = build_model("static_one", synth.state_dict("static_one"))
    assert _guard_flag(_blob(model)) == 0
    lg, mk = _check(model, torch.from_numpy(pts_np).cuda(), 3, "C2")
    assert bool(torch.isfinite(lg).all())


def test_dynamic_fp32_full_launch_equals_the_dense_family_on_every_row():
    """DynamicModel's segmentation net: c_in = 4, 1024 items x 5120 points (3 items per latency launch)"""
    p, _, _, _ = synth.dynamic_items(1024)
    model = build_model("dynamic", synth.state_dict("dynamic"))
    _check(model, torch.from_numpy(p).cuda(), 4, "Dynamic_fp32")


@pytest.mark.parametrize("B,N", [(600, 1), (520, 33), (1200, 77), (300, 1000), (131, 1023), (40, 2049), (20, 4096)])
def test_ragged_point_counts(B, N):
    """N from 1 to 4096, not a multiple of 32 / 128: a wave's last tile replicates the crop's last point, whole waves
    of a workgroup have no tile"""
    pts_np, _, _ = synth.static_crops(B, N, seed=N)
    model = build_model("static_one", synth.state_dict("static_one", seed=7))
    _check(model, torch.from_numpy(pts_np).cuda(), 3, f"ragged {B}x{N}")


def _with_dconv1_bias(seed, shift):
    """synth weights with `shift` (512,) added to dconv1's folded bias (the BN's beta)"""
    sd = dict(synth.state_dict("static_one", seed=seed))
    sd["ins_seg.dbn1.bias"] = (np.asarray(sd["ins_seg.dbn1.bias"]).astype(np.float32) + shift.astype(np.float32))
    return sd


def test_every_channel_dead():
    """dconv1's bias far below zero: relu(dconv1) is +0 everywhere, no chunk has a compact k-step, dconv2 is its bias"""
    pts_np, _, _ = synth.static_crops(96, 1024, seed=93)
    model = build_model("static_one", _with_dconv1_bias(93, np.full(512, -1e6)))
    _check(model, torch.from_numpy(pts_np).cuda(), 3, "all dead")


def test_nothing_dead():
    """dconv1's bias far above zero: no entry of the crops' dconv1 term is negative, every tile runs the dense body"""
    pts_np, _, _ = synth.static_crops(96, 1024, seed=94)
    model = build_model("static_one", _with_dconv1_bias(94, np.full(512, 1e6)))
    _check(model, torch.from_numpy(pts_np).cuda(), 3, "nothing dead")


def test_fully_live_chunks_inside_a_compacted_tile():
    """chunks 0..7 fully live, chunks 8..15 dead: the crop's term has 256 negative entries, so its tiles take the compacted
    body, whose first eight chunks run the register path on the fragment stream and whose last eight have no k-step"""
    shift = np.full(512, -1e6)
    shift[:256] = 1e6
    pts_np, _, _ = synth.static_crops(96, 1024, seed=89)
    model = build_model("static_one", _with_dconv1_bias(89, shift))
    _check(model, torch.from_numpy(pts_np).cuda(), 3, "dense chunks in a compacted tile")


@pytest.mark.parametrize("extra", [0, 1])
def test_odd_live_counts_in_every_chunk(extra):
    """chunk c keeps 2 c + 1 channels alive in every tile (1, 3, ... 31 of 32, at scattered places) and loses the others:
    a channel waits at every second chunk seam. extra = 1 revives the last chunk's one dead channel: a fully live chunk
    behind a waiting channel (compacted, 16 k-steps), 257 live channels, the last one paired with the row of zeros"""
    rng = np.random.default_rng(95)
    shift = np.full(512, -1e6)
    for c in range(16):
        shift[32 * c + rng.permutation(32)[:2 * c + 1]] = 1e6
    if extra:
        shift[32 * 15:] = 1e6
    pts_np, _, _ = synth.static_crops(96, 1024, seed=95)
    model = build_model("static_one", _with_dconv1_bias(95, shift))
    _check(model, torch.from_numpy(pts_np).cuda(), 3, f"odd live counts + {extra}")


@pytest.mark.parametrize("channel", [0, 37, 511])
def test_single_live_channel(channel):
    """one live channel in the whole layer: it waits through every later chunk and is paired with the row of zeros"""
    shift = np.full(512, -1e6)
    shift[channel] = 1e6
    pts_np, _, _ = synth.static_crops(96, 1024, seed=96)
    model = build_model("static_one", _with_dconv1_bias(96, shift))
    _check(model, torch.from_numpy(pts_np).cuda(), 3, f"single live channel {channel}")


def test_mixed_tiles_inside_a_crop():
    """crops whose second half repeats one far-away point: tiles of one crop see different live sets (dconv1's per-point
    part differs), some tiles of a crop are dense and others compacted"""
    pts_np, _, _ = synth.static_crops(96, 1024, seed=97)
    p = pts_np.copy()
    p[::2, 512:] = p[::2, 511:512] * np.float32(50.0)
    p[1::4, 100:132] *= np.float32(300.0)
    shift = np.zeros(512)
    shift[::3] = 40.0                                      # a third of the channels live almost everywhere
    model = build_model("static_one", _with_dconv1_bias(97, shift))
    _check(model, torch.from_numpy(p).cuda(), 3, "mixed tiles")


def test_minus_zero_bias_takes_the_dense_path():
    """a folded dconv2 bias with the bit pattern of -0 sets the blob's flag (checked on the packed blob) and the outputs
    equal the latency family's. The outputs alone cannot show that the kernel honours the flag here: the sign of a zero
    accumulator never reaches an output bit (DESIGN.md "Compacted dconv2"); the Inf case below can."""
    sd = dict(synth.state_dict("static_one", seed=98))
    gamma = np.asarray(sd["ins_seg.dbn2.weight"]).astype(np.float32).copy()
    beta = np.asarray(sd["ins_seg.dbn2.bias"]).astype(np.float32).copy()
    bias = np.asarray(sd["ins_seg.dconv2.bias"]).astype(np.float32).copy()
    gamma[5] = -abs(gamma[5]) - np.float32(0.1)            # (b - mean) * s + beta = (+0) * (negative) + (-0) = -0
    beta[5] = np.float32(-0.0)
    bias[5] = np.asarray(sd["ins_seg.dbn2.running_mean"])[5]
    sd["ins_seg.dbn2.weight"], sd["ins_seg.dbn2.bias"], sd["ins_seg.dconv2.bias"] = gamma, beta, bias
    model = build_model("static_one", sd)
    assert _guard_flag(_blob(model)) == 1
    pts_np, _, _ = synth.static_crops(96, 1024, seed=98)
    _check(model, torch.from_numpy(pts_np).cuda(), 3, "-0 bias")


def test_infinite_weight_takes_the_dense_path():
    """an Inf dconv2 weight sets the blob's flag. The two input channels that carry the Inf weights are dead in every tile
    (dconv1 bias -1e6) and 254 others with them, so the crops qualify for the compacted body: a kernel that ignored the
    flag would skip the two terms, while the dense chain computes 0 * Inf = NaN in output rows 3 and 200"""
    shift = np.zeros(512)
    shift[np.random.default_rng(99).permutation(512)[:254]] = -1e6
    shift[17] = shift[500] = -1e6
    sd = _with_dconv1_bias(99, shift)
    wt = np.asarray(sd["ins_seg.dconv2.weight"]).astype(np.float32).copy()
    wt[3, 17, 0] = np.inf
    wt[200, 500, 0] = -np.inf
    sd["ins_seg.dconv2.weight"] = wt
    model = build_model("static_one", sd)
    assert _guard_flag(_blob(model)) == 1
    pts_np, _, _ = synth.static_crops(96, 1024, seed=99)
    _check(model, torch.from_numpy(pts_np).cuda(), 3, "Inf weight")


def test_non_finite_crops_inside_a_large_batch():
    """NaN / Inf coordinates: every logit of the crop is the quiet NaN and its mask is empty, as from the dense kernels; its
    neighbours are untouched"""
    B, N = 80, 1024
    pts_np, _, _ = synth.static_crops(B, N, seed=92)
    p = pts_np.copy()
    p[1, 7, 0] = np.nan
    p[3, 0, 2] = np.inf
    p[4, N - 1, 1] = -np.inf
    p[79, 500, 1] = np.nan
    model = build_model("static_one", synth.state_dict("static_one", seed=92))
    lg, mk = _check(model, torch.from_numpy(p).cuda(), 3, "non-finite")
    bad = [1, 3, 4, 79]
    good = [b for b in range(B) if b not in bad]
    assert bool(torch.isnan(lg[bad]).all()) and bool(torch.isfinite(lg[good]).all()) and int(mk[bad].sum()) == 0
    clean, mk_clean = _check(model, torch.from_numpy(pts_np).cuda(), 3, "clean")
    assert torch.equal(clean[good], lg[good]) and torch.equal(mk_clean[good], mk[good])


def test_shards_equal_the_whole():
    """one launch of 96 crops against two of 48 (all three in the throughput family): a crop's bits do not depend on
    which workgroup, XCD or launch it falls into"""
    pts_np, _, _ = synth.static_crops(96, 1024, seed=90)
    model = build_model("static_one", synth.state_dict("static_one", seed=90))
    w = _blob(model)
    x = torch.from_numpy(pts_np).cuda().transpose(2, 1)
    g, lg, mk = _forward(w, 3, x)
    for lo in (0, 48):
        g2, lg2, mk2 = _forward(w, 3, x[lo:lo + 48])
        assert _same_bits(g2, g[lo:lo + 48]) and _same_bits(lg2, lg[lo:lo + 48]) and torch.equal(mk2, mk[lo:lo + 48])
