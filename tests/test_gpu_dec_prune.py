"""dconv1's channels that are dead for a whole crop (DESIGN.md "Crop-dead channels of dconv1"): the screened encoder's bound, the
plan kernel's flags and the decoder that runs dconv1 over the plan, on the device.

Every batch is the smallest that reaches the screened encoder and the throughput decoder: more than 65,536 points and more
than 512 tiles (520 crops x 128 points; 65 x 1025 for the ragged case). The plan is switched off per call with
DAL3_BCN_NO_DEC_PLAN; both calls run the same kernels otherwise, and the outputs must have the same bits."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import dec_prune_model as M
from _common import build_model, synth

hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 288, 448, 449, 511, 512]     # live channels; 448 / 449: MIN_DEAD and MIN_DEAD - 1 flags


def _blob(model):
    return model._cache.get("ins_seg", model.ins_seg, hip.HEAD_INS_SEG)


def _forward(w, c_in, x, flags=0):
    """x: (B, c_in, N) view on the GPU -> (global feature, logits, mask, workspace) of one dal3_ins_seg_forward launch"""
    lib = hip.lib()
    B, _, N = x.shape
    assert B * N > 65536 and B * ((N + 31) // 32) > 512, "the launch must reach the screened encoder and the throughput decoder"
    ws = torch.zeros(lib.dal3_ins_seg_workspace_bytes(B), dtype=torch.uint8, device="cuda")
    g = torch.empty((B, 1024), device="cuda")
    lg = torch.empty((B, N, 2), device="cuda")
    mk = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    v = hip.bcn(x)
    v.flags |= flags
    hip.check(lib.dal3_ins_seg_forward(hip.ptr(w), hip.F32, c_in, v, B, N, hip.ptr(lg), hip.ptr(mk), hip.ptr(g),
                                       hip.ptr(ws), ws.numel(), hip.stream()))
    return g, lg, mk, ws


def _plan(ws, B):
    """the plan a forward left in its workspace: U (B,512) fp32 by channel (NaN where nothing was seen), X (B,), the lists
    (B,640), the gathered terms (B,512), the chunk counts (B,) — on the CPU"""
    off = (C.c_size_t * 4)()
    md = C.c_int(0)
    hip.check(hip.lib().dal3_ins_seg_plan_layout(B, off, C.byref(md)))
    assert md.value == M.MIN_DEAD
    take = lambda o, n, dt: ws[o:o + 4 * n].view(dt).cpu()
    pr = take(off[0], B * 513, torch.int32).view(B, 513).numpy().view(np.uint32)
    keys = pr[:, :512]
    bits = np.where(keys >> 31, keys ^ np.uint32(0x80000000), ~keys)
    U = bits.view(np.float32).copy()
    X = pr[:, 512].copy().view(np.float32)
    lst = take(off[1], B * M.PLAN_LD, torch.int32).view(B, M.PLAN_LD).numpy().astype(np.int64)
    gbc = take(off[2], B * 512, torch.float32).view(B, 512).numpy()
    nch = take(off[3], B, torch.int32).numpy()
    return U, X, lst, gbc, nch, keys


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _on_equals_off(model, x, c_in, what):
    w = _blob(model)
    g1, lg1, mk1, ws = _forward(w, c_in, x)
    g0, lg0, mk0, _ = _forward(w, c_in, x, hip.BCN_NO_DEC_PLAN)
    assert _same_bits(g1, g0), what
    same = _same_bits(lg1, lg0)
    if not same:
        diff = (lg1.view(torch.int32) != lg0.view(torch.int32)).any(2)
        print(f"{what}: crops {torch.nonzero(diff.any(1)).flatten()[:8].tolist()} differ, {int(diff.sum())} points")
    assert same and torch.equal(mk1, mk0), what
    return g1, lg1, mk1, ws


def _layer(conv_w, conv_b, bn, c_in, c_out, x, relu=1):
    """dal3_shared_mlp_layer on raw tensors (bn: dict with weight / bias / running_mean / running_var) -> (B,N,c_out)"""
    lib = hip.lib()
    B, _, N = x.shape
    L = hip.Layer(hip.ptr(conv_w), hip.ptr(conv_b), hip.ptr(bn["weight"]), hip.ptr(bn["bias"]), hip.ptr(bn["running_mean"]),
                  hip.ptr(bn["running_var"]), c_in, c_out)
    ws = torch.empty(lib.dal3_shared_mlp_layer_workspace_bytes(c_in, c_out), dtype=torch.uint8, device="cuda")
    y = torch.empty((B, N, c_out), device="cuda")
    hip.check(lib.dal3_shared_mlp_layer(C.byref(L), relu, hip.bcn(x), B, N, hip.ptr(y), hip.ptr(ws), ws.numel(), hip.stream()))
    return y


def _device_x2(sd, x, c_in):
    dev = lambda k: torch.as_tensor(np.asarray(sd[k])).float().cuda().contiguous()
    bn = lambda n: {k: dev(f"ins_seg.{n}.{k}") for k in ("weight", "bias", "running_mean", "running_var")}
    x1 = _layer(dev("ins_seg.conv1.weight"), dev("ins_seg.conv1.bias"), bn("bn1"), c_in, 64, x)
    return _layer(dev("ins_seg.conv2.weight"), dev("ins_seg.conv2.bias"), bn("bn2"), 64, 64, x1.transpose(2, 1))


def _device_dconv1(sd, x2, gb_row, b):
    """the device's own dense dconv1 of crop b: relu(W1a' x2 + gb), the term planted as the folded bias (conv bias = the
    BN's mean, so that (bias - mean) * s + beta is beta = gb bit for bit) -> (N,512)"""
    dev = lambda k: torch.as_tensor(np.asarray(sd[k])).float().cuda()
    w = dev("ins_seg.dconv1.weight")[:, :64].contiguous()
    bn = {k: dev(f"ins_seg.dbn1.{k}") for k in ("weight", "running_mean", "running_var")}
    bn["bias"] = gb_row.contiguous()
    return _layer(w, bn["running_mean"].clone(), bn, 64, 512, x2[b:b + 1].transpose(2, 1))[0]


def _global_bias(w, g):
    B = g.shape[0]
    gb = torch.empty((B, 512), device="cuda")
    hip.check(hip.lib().dal3_ins_seg_global_bias(hip.ptr(w), hip.F32, hip.ptr(g), B, hip.ptr(gb), hip.stream()))
    return gb


def _check_bound_and_flags(sd, pts_np, c_in, crops):
    model = build_model("static_one" if c_in == 3 else "dynamic", sd)
    x = torch.from_numpy(pts_np).cuda().transpose(2, 1)
    B = x.shape[0]
    g, lg, mk, ws = _on_equals_off(model, x, c_in, "bound")
    U, X, lst, gbc, nch, keys = _plan(ws, B)
    gb = _global_bias(_blob(model), g)
    x2 = _device_x2(sd, x, c_in)                            # (B,N,64)
    tsd = {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}
    w1, _ = M._fold(tsd, "ins_seg", "dconv1", "dbn1")
    w1a = w1[:, :64].contiguous()
    P, Q = M.coefficients(w1a)
    assert (keys != 0).all() and np.isfinite(X).all() and (nch > 0).any()
    x2c = x2.cpu()
    for b in crops:
        xb = x2c[b].T.contiguous()                          # (64,N)
        # U dominates the exact maximum minus the bound (and lies below it plus the bound): float64 on the fp32 operands
        # stands in for the chain from +0, whose own rounding the bound covers; the folded weights are the oracle's, whose
        # last-bit differences from the packer's fold are covered by the 1e-6 of the products' sum
        exact = (w1a.double() @ xb.double())
        slack = 1e-6 * (w1a.double().abs() @ xb.double().abs()).amax(1)
        E = float(X[b]) * P + Q
        top = exact.amax(1)
        assert bool((torch.from_numpy(U[b]).double() >= top - E - slack).all()), b
        assert bool((torch.from_numpy(U[b]).double() <= top + E + slack).all()), b
        assert float(X[b]) >= float(xb.double().norm(dim=0).max())
        # the flags are a subset of the channels the device's own dense dconv1 leaves all-zero
        n = int((lst[b] < M.NULL_K).sum())
        flagged = np.ones(512, bool)
        flagged[M.CHAIN[lst[b, :n]]] = False
        y = _device_dconv1(sd, x2, gb[b], b)
        dead = (y.view(torch.int32) == 0).all(0).cpu().numpy()
        assert not (flagged & ~dead).any(), (b, np.nonzero(flagged & ~dead)[0][:8])
        M.judge_plan(lst[b], gbc[b], int(nch[b]) if 512 - n >= M.MIN_DEAD else 0, flagged, gb[b].cpu().numpy())
        assert (nch[b] > 0) == (512 - n >= M.MIN_DEAD)
    return U, X, lst, nch


def test_bound_and_flags_on_bench_weights():
    """520 crops x 128 points of the bench's generator and weights"""
    pts_np, _, _ = synth.static_crops(520, 128)
    sd = synth.state_dict("static_one")
    U, X, lst, nch = _check_bound_and_flags(sd, pts_np, 3, [0, 1, 7, 260, 519])
    share = 1.0 - float((lst[:, :512] < M.NULL_K).mean())
    print(f"flagged share {share:.4f}, chunk counts {sorted(set(nch.tolist()))}")
    assert share > 0.3                                      # (128 of a crop's points: more channels are dead than at 1024)


def test_ragged_crops():
    """65 crops x 1025 points: a crop's last wave holds one point and replicates it"""
    pts_np, _, _ = synth.static_crops(65, 1025, seed=11)
    _check_bound_and_flags(synth.state_dict("static_one", seed=7), pts_np, 3, [0, 64])


def test_four_input_channels():
    """DynamicModel's segmentation net, c_in = 4"""
    p, _, _, _ = synth.dynamic_items(520, n_per_frame=26)   # 5 x 26 = 130 points per item
    _check_bound_and_flags(synth.state_dict("dynamic"), p, 4, [0, 519])


def _planted(seed):
    """Weights and a batch in which the live counts of COUNTS occur side by side: 13 classes of crops (one base crop each,
    crop b is class b % 13). One channel j of the pooled feature separates the classes (z_0 < ... < z_12, measured on the
    device: the encoder does not depend on dconv1); dconv1's column of that channel and its bias are planted so that channel
    c's term is A (z - tau_c), with tau_c between two classes' values: class i keeps exactly COUNTS[i] channels (nested sets,
    scattered over the chunks) and every term is at least 1e6 away from zero, as with the A/B tool's --dead-frac."""
    n_cls = len(COUNTS)
    base, _, _ = synth.static_crops(n_cls, 128, seed=seed)
    sd = dict(synth.state_dict("static_one", seed=seed))
    model = build_model("static_one", sd)
    B = 520
    pts_np = base[np.arange(B) % n_cls]
    x = torch.from_numpy(pts_np).cuda().transpose(2, 1)
    g, _, _, _ = _forward(_blob(model), 3, x, hip.BCN_NO_DEC_PLAN)
    z_all = g[:n_cls].cpu().numpy().astype(np.float64)      # (13,1024)
    srt = np.sort(z_all, axis=0)
    j = int(np.argmax(np.diff(srt, axis=0).min(0)))         # the channel whose closest two classes are farthest apart
    z = z_all[:, j]
    order = np.argsort(z)                                   # class of rank i
    gap = float(np.diff(z[order]).min())
    assert gap > 1e-3 * float(np.abs(z).max()), "no channel of the pooled feature separates the base crops"
    mid = (z[order][1:] + z[order][:-1]) / 2
    tau = np.empty(512)
    perm = np.random.default_rng(seed).permutation(512)
    # rank i keeps COUNTS[i] channels: perm[:COUNTS[i]] have tau below z of rank i
    for i in range(n_cls):
        lo = COUNTS[i - 1] if i else 0
        tau[perm[lo:COUNTS[i]]] = mid[i - 1] if i else z[order][0] - gap
    A = 4e6 / gap
    s = np.asarray(sd["ins_seg.dbn1.weight"], np.float64) / np.sqrt(np.asarray(sd["ins_seg.dbn1.running_var"], np.float64) + 1e-5)
    wt = np.asarray(sd["ins_seg.dconv1.weight"]).astype(np.float32).copy()
    wt[:, 64 + j, 0] += (A / s).astype(np.float32)
    sd["ins_seg.dconv1.weight"] = wt
    sd["ins_seg.dbn1.bias"] = (np.asarray(sd["ins_seg.dbn1.bias"], np.float64) - A * tau).astype(np.float32)
    live_of_crop = np.empty(B, np.int64)
    rank = np.argsort(order)
    live_of_crop[:] = np.array(COUNTS)[rank[np.arange(B) % n_cls]]
    return sd, pts_np, live_of_crop


def test_planted_live_counts_side_by_side():
    """odd chunk counts, every length of the last group, a leftover carried across the last group, nothing live, everything
    live, MIN_DEAD - 1 and MIN_DEAD flags in neighbouring crops: logits and mask with the plan on and off"""
    sd, pts_np, live = _planted(21)
    model = build_model("static_one", sd)
    x = torch.from_numpy(pts_np).cuda().transpose(2, 1)
    g, lg, mk, ws = _on_equals_off(model, x, 3, "planted counts")
    U, X, lst, gbc, nch, _ = _plan(ws, 520)
    got = (lst[:, :512] < M.NULL_K).sum(1)
    assert np.array_equal(got, live), (got[:13], live[:13])
    want = np.where(512 - live < M.MIN_DEAD, 0, np.maximum(2, ((live + 31) // 32 + 1) & ~1))
    assert np.array_equal(nch, want)
    assert set(want.tolist()) >= {0, 2, 4, 10, 14}
    assert bool(torch.isfinite(lg).all())


def test_non_finite_crop_between_finite_ones():
    pts_np, _, _ = synth.static_crops(520, 128, seed=5)
    p = pts_np.copy()
    p[100, 7, 0] = np.nan
    p[101, 0, 2] = np.inf
    p[300] *= np.float32(1e4)                               # activations beyond fp16's range: no bound, nothing flagged
    model = build_model("static_one", synth.state_dict("static_one", seed=5))
    x = torch.from_numpy(p).cuda().transpose(2, 1)
    g, lg, mk, ws = _on_equals_off(model, x, 3, "non-finite")
    U, X, lst, gbc, nch, _ = _plan(ws, 520)
    for b in (100, 101, 300):
        assert nch[b] == 0 and (lst[b, :512] == np.arange(512)).all(), b
    assert np.isinf(X[300]) and nch[99] > 0 and nch[102] > 0
    assert bool(torch.isnan(lg[[100, 101]]).all()) and int(mk[[100, 101]].sum()) == 0
    clean = torch.from_numpy(pts_np).cuda().transpose(2, 1)
    _, lg2, mk2, _ = _forward(_blob(model), 3, clean)
    keep = [b for b in range(520) if b not in (100, 101, 300)]
    assert _same_bits(lg[keep], lg2[keep]) and torch.equal(mk[keep], mk2[keep])
