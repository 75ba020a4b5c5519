#!/usr/bin/env python3
"""A/B timing of library builds in ONE process (cdna guide rule 24): interleaved rounds of the
three shared-MLP kernels, median and min per build, outputs cross-checked against the first build.
`seg` is dal3_ins_seg_forward — encoder, per-crop FC, the decoder's plan where the build has one, decoder — as a step runs
them (`dec` alone is the stand-alone entry, which never has a plan); `seg0` the same call with DAL3_BCN_NO_DEC_PLAN.
`enc2` / `seg2` are `enc` / `seg` with DAL3_BCN_NO_ENC_RESIDENT (the screened encoder's two launches) where the build knows
that flag, the same call as `enc` / `seg` where it does not; `head2` likewise is `head` with DAL3_BCN_NO_HEAD_RESIDENT (the
screened point head's two launches). `dec1` / `seg1` are `dec` / `seg` with DAL3_BCN_NO_DEC_PAIR (the decoder with one wave
per tile) where the build knows that flag; their logits and masks are cross-checked too. A -DDAL3_SCREEN_COUNT build prints the screen's counters of one `seg` and one `seg2` call.

  python tools/ab_kernels.py build_a.so build_b.so ... [--B 4096] [--N 1024] [--rounds 7]
"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hip = importlib.import_module("3dal_pytorch_amd._hip")
synth = importlib.import_module("3dal_pytorch_amd.synth")
sm = importlib.import_module("3dal_pytorch_amd.static_model")

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="+")
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--N", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--dtype", type=int, default=0, help="0 fp32, 1 bf16, 2 fp16")
ap.add_argument("--dbn1-shift", type=float, default=0.0,
                help="added to dconv1's folded bias: +1e6 = no dead channel in dconv2's input, -1e6 = every channel dead")
ap.add_argument("--dead-frac", type=float, default=None,
                help="dconv1's folded bias -1e6 on this fraction of the 512 channels (scattered), +1e6 on the others: exactly "
                     "that share of dconv2's input is dead in every tile")
args = ap.parse_args()
B, N = args.B, args.N
DT = args.dtype
dev = torch.device("cuda:0")


def load(path):
    h = C.CDLL(os.path.abspath(path))
    for name, (res, a) in hip.SIGNATURES.items():
        if not hasattr(h, name):                      # an older build may predate some entry points
            continue
        fn = getattr(h, name)
        fn.restype, fn.argtypes = res, a
    return h


model = sm.StaticModelOneBoxEst()
sd = dict(synth.state_dict("static_one"))
if args.dead_frac is not None:
    shift = np.full(512, 1e6, np.float32)
    shift[np.random.default_rng(0).permutation(512)[:int(round(args.dead_frac * 512))]] = -1e6
    sd["ins_seg.dbn1.bias"] = sd["ins_seg.dbn1.bias"] + shift
if args.dbn1_shift:
    sd["ins_seg.dbn1.bias"] = sd["ins_seg.dbn1.bias"] + np.float32(args.dbn1_shift)
model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
model = model.to(dev).eval()
pts_np, init_np, _ = synth.static_crops(min(B, 512), N)
reps = (B + pts_np.shape[0] - 1) // pts_np.shape[0]
pts = torch.from_numpy(pts_np).to(dev).repeat(reps, 1, 1)[:B].contiguous().transpose(2, 1)
obj = pts.transpose(2, 1)[:, :512, :].contiguous().transpose(2, 1)
x, xo = hip.bcn(pts), hip.bcn(obj)
st = hip.stream()
names = [os.path.basename(p) for p in args.libs]
if len(set(names)) < len(names):                          # the same file name in several trees: tell them apart by their paths
    names = [os.path.relpath(p) for p in args.libs]
libs = [(n, load(p)) for n, p in zip(names, args.libs)]
state = []
for name, lib in libs:
    need = C.c_size_t(0)
    def pack(kind, pairs):
        arr = (hip.Layer * len(pairs))(*[hip.layer_struct(c, b) for c, b in pairs])
        lib.dal3_pack_weights(kind, arr, len(pairs), DT, None, C.byref(need), None)
        buf = torch.zeros(need.value, dtype=torch.uint8, device=dev)
        rc = lib.dal3_pack_weights(kind, arr, len(pairs), DT, hip.ptr(buf), C.byref(need), st)
        assert rc == 0, lib.dal3_last_error()
        return buf
    w_seg = pack(hip.HEAD_INS_SEG, model.ins_seg.pairs())
    w_box = pack(hip.HEAD_STATIC_BOX_EST, model.box_est.pairs())
    g = torch.zeros((B, 1024), device=dev)
    gb = torch.empty((B, 512), device=dev)
    logits = torch.empty((B, N, 2), device=dev)
    mask = torch.empty((B, N), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.dal3_point_head_workspace_bytes(B), dtype=torch.uint8, device=dev)
    bp = torch.empty((B, 39), device=dev)
    ws_seg = torch.zeros(lib.dal3_ins_seg_workspace_bytes(B), dtype=torch.uint8, device=dev)
    lg_seg, mk_seg, g_seg = torch.empty_like(logits), torch.empty_like(mask), torch.empty_like(g)
    d = dict(w_seg=w_seg, w_box=w_box, g=g, gb=gb, logits=logits, mask=mask, ws=ws, bp=bp, ws_seg=ws_seg, lg_seg=lg_seg,
             mk_seg=mk_seg, g_seg=g_seg, has_plan=hasattr(lib, "dal3_ins_seg_plan_layout"))

    def seg(lib=lib, d=d, flags=0):
        v = hip.bcn(pts)
        v.flags |= flags
        return lib.dal3_ins_seg_forward(hip.ptr(d["w_seg"]), DT, 3, v, B, N, hip.ptr(d["lg_seg"]), hip.ptr(d["mk_seg"]),
                                        hip.ptr(d["g_seg"]), hip.ptr(d["ws_seg"]), d["ws_seg"].numel(), st)
    d["seg"] = seg
    d["seg0"] = (lambda seg=seg: seg(flags=hip.BCN_NO_DEC_PLAN)) if d["has_plan"] else seg
    d["has_res"] = hasattr(lib, "dal3_ins_seg_encoder_route")
    two = hip.BCN_NO_ENC_RESIDENT if d["has_res"] else 0
    d["seg2"] = lambda seg=seg, two=two: seg(flags=two)
    x2 = hip.bcn(pts)
    x2.flags |= two
    if d["has_res"]:
        print(f"{name}: encoder route {lib.dal3_ins_seg_encoder_route(B, N, 0)} "
              f"(with DAL3_BCN_NO_ENC_RESIDENT {lib.dal3_ins_seg_encoder_route(B, N, two)})")
    # g is zeroed before EVERY encode, as a step does (nonfinite_rows_kernel): the screened fp32 encoder's second launch
    # reads its thresholds from g, and on a g that already holds the final maxima it would find fewer candidates than it
    # ever does in a step. (The fill is a 16.8-MB memset, ~5 us, the same for every build.)
    d["enc"] = lambda lib=lib, d=d, x=x: (d["g"].zero_(), lib.dal3_ins_seg_encode(hip.ptr(d["w_seg"]), DT, 3, x, B, N, hip.ptr(d["g"]), st))[1]
    d["enc2"] = lambda enc=d["enc"], x2=x2: enc(x=x2)
    d["dec"] = lambda lib=lib, d=d: lib.dal3_ins_seg_decode(hip.ptr(d["w_seg"]), DT, 3, x, B, N, hip.ptr(d["gb"]),
                                                            hip.ptr(d["logits"]), hip.ptr(d["mask"]), st)
    d["head"] = lambda lib=lib, d=d: lib.dal3_point_head_forward(hip.HEAD_STATIC_BOX_EST, hip.ptr(d["w_box"]), DT, xo, B, 512,
                                                                 hip.ptr(d["bp"]), 39, hip.ptr(d["ws"]), d["ws"].numel(), st)
    d["has_pair"] = hasattr(lib, "dal3_ins_seg_decode_route")
    one = hip.BCN_NO_DEC_PAIR if d["has_pair"] else 0
    x1 = hip.bcn(pts)
    x1.flags |= one
    d["logits1"], d["mask1"] = torch.empty_like(logits), torch.empty_like(mask)
    d["dec1"] = lambda lib=lib, d=d, x1=x1: lib.dal3_ins_seg_decode(hip.ptr(d["w_seg"]), DT, 3, x1, B, N, hip.ptr(d["gb"]),
                                                                    hip.ptr(d["logits1"]), hip.ptr(d["mask1"]), st)
    d["seg1"] = lambda seg=seg, one=one: seg(flags=one)
    if d["has_pair"]:
        print(f"{name}: decoder route {lib.dal3_ins_seg_decode_route(hip.ptr(w_seg), B, N, 0)} "
              f"(with DAL3_BCN_NO_DEC_PAIR {lib.dal3_ins_seg_decode_route(hip.ptr(w_seg), B, N, one)})")
    d["has_head_res"] = hasattr(lib, "dal3_point_head_route")
    xo2 = hip.bcn(obj)
    xo2.flags |= hip.BCN_NO_HEAD_RESIDENT if d["has_head_res"] else 0
    d["bp2"] = torch.empty((B, 39), device=dev)
    d["head2"] = lambda lib=lib, d=d, xo2=xo2: lib.dal3_point_head_forward(hip.HEAD_STATIC_BOX_EST, hip.ptr(d["w_box"]), DT, xo2, B, 512,
                                                                          hip.ptr(d["bp2"]), 39, hip.ptr(d["ws"]), d["ws"].numel(), st)
    if d["has_head_res"]:
        print(f"{name}: point head route {lib.dal3_point_head_route(hip.HEAD_STATIC_BOX_EST, B, 512, 0)} "
              f"(with DAL3_BCN_NO_HEAD_RESIDENT {lib.dal3_point_head_route(hip.HEAD_STATIC_BOX_EST, B, 512, hip.BCN_NO_HEAD_RESIDENT)})")
    assert d["enc"]() == 0, lib.dal3_last_error()
    assert lib.dal3_ins_seg_global_bias(hip.ptr(w_seg), DT, hip.ptr(g), B, hip.ptr(gb), st) == 0
    if hasattr(lib, "dal3_debug_dec_counts"):         # a -DDAL3_DEC_COUNT build: what the compacted dconv2 saw in ONE launch
        cnt = (C.c_ulonglong * 12)()
        lib.dal3_debug_dec_counts(cnt, 1)
    assert d["dec"]() == 0 and d["head"]() == 0, lib.dal3_last_error()
    if hasattr(lib, "dal3_debug_dec_counts"):
        torch.cuda.synchronize()
        lib.dal3_debug_dec_counts(cnt, 1)
        tiles, dense, comp, steps, live, sp_tiles = (int(v) for v in cnt[:6])
        print(f"{name}: decode tiles {tiles} ({sp_tiles} in the compacted body), dense chunks {dense}, compacted chunks {comp}, compact k-steps {steps} "
              f"({(steps + 16 * dense) / (256.0 * tiles):.4f} of the dense k-steps), live channels {live / (512.0 * tiles):.4f}")
        s3, l3, s4, l4 = (int(v) for v in cnt[6:10])      # the queue layers, tiles of the compacted body only
        if sp_tiles:
            print(f"{name}: dconv3 compact k-steps {s3} ({s3 / (128.0 * sp_tiles):.4f} of dense), live rows {l3 / (256.0 * sp_tiles):.4f}; "
                  f"dconv4 compact k-steps {s4} ({s4 / (64.0 * sp_tiles):.4f} of dense), live rows {l4 / (128.0 * sp_tiles):.4f}")
    assert d["seg0"]() == 0, lib.dal3_last_error()
    torch.cuda.synchronize()
    d["lg_seg0"], d["mk_seg0"] = d["lg_seg"].clone(), d["mk_seg"].clone()
    if hasattr(lib, "dal3_debug_dec_counts"):
        lib.dal3_debug_dec_counts(cnt, 1)
    assert d["seg"]() == 0, lib.dal3_last_error()
    if hasattr(lib, "dal3_debug_dec_counts"):         # the same counts for the decoder inside the whole call (with its plan)
        torch.cuda.synchronize()
        lib.dal3_debug_dec_counts(cnt, 1)
        tiles, dense, comp, steps, live, sp_tiles = (int(v) for v in cnt[:6])
        print(f"{name}: ins_seg_forward: decode tiles {tiles} ({sp_tiles} in the compacted body), dense chunks {dense}, compacted chunks "
              f"{comp} ({comp / max(sp_tiles, 1):.3f} per compacted tile), compact k-steps {steps} ({steps / max(sp_tiles, 1):.3f} per compacted tile), "
              f"live channels among the computed ones {live / max(32.0 * (comp + dense), 1):.4f}")
    if hasattr(lib, "dal3_debug_screen_counts") and DT == 0:
        sc = (C.c_ulonglong * 8)()
        for kind in ("seg", "seg2") if d["has_res"] else ("seg",):
            torch.cuda.synchronize()
            lib.dal3_debug_screen_counts(sc, 1)
            assert d[kind]() == 0, lib.dal3_last_error()
            torch.cuda.synchronize()
            lib.dal3_debug_screen_counts(sc, 1)
            waves, rng, ovf, cand, rounds = (int(v) for v in sc[:5])
            tiles = B * ((N + 63) // 64) * 2
            print(f"{name} {kind} {B}x{N}: waves {waves}, dense for range {rng}, list overflow {ovf}, candidates {cand} = "
                  f"{cand / tiles:.1f} per tile, recompute rounds {rounds} = {rounds / tiles:.2f} per tile")
        assert d["seg"]() == 0, lib.dal3_last_error()
    if d["has_plan"] and DT == 0:
        off, md = (C.c_size_t * 4)(), C.c_int(0)
        assert lib.dal3_ins_seg_plan_layout(B, off, C.byref(md)) == 0
        torch.cuda.synchronize()
        nch = ws_seg[off[3]:off[3] + 4 * B].view(torch.int32).cpu().numpy()
        lst = ws_seg[off[1]:off[1] + 4 * 640 * B].view(torch.int32).view(B, 640)[:, :512].cpu().numpy()
        live = (lst < 512).sum(1)
        print(f"{name}: plan: {int((nch > 0).sum())} of {B} crops, flagged share {1 - live.mean() / 512:.4f}, live channels "
              f"{int(live.min())} - {int(live.max())}, chunks run per tile {np.where(nch > 0, nch, 16).mean():.2f} of 16")
    state.append(d)
torch.cuda.synchronize()
ref = state[0]
for (name, _), d in zip(libs, state):
    same = (torch.equal(d["g"], ref["g"]), torch.equal(d["logits"].view(torch.int32), ref["logits"].view(torch.int32)),
            torch.equal(d["mask"], ref["mask"]), torch.equal(d["bp"], ref["bp"]))
    assert d["enc2"]() == 0 and d["seg2"]() == 0 and d["head2"]() == 0, _.dal3_last_error()
    torch.cuda.synchronize()
    print(f"{name}: point head under DAL3_BCN_NO_HEAD_RESIDENT bitwise-equal to the first build (box_pred) = "
          f"{torch.equal(d['bp2'].view(torch.int32), ref['bp'].view(torch.int32))}")
    print(f"{name}: two-launch encoder bitwise-equal to the first build (g of enc2, g / logits / mask of seg2) = "
          f"{(torch.equal(d['g'], ref['g']), torch.equal(d['g_seg'].view(torch.int32), ref['g_seg'].view(torch.int32)), torch.equal(d['lg_seg'].view(torch.int32), ref['lg_seg0'].view(torch.int32)), torch.equal(d['mk_seg'], ref['mk_seg0']))}")
    bits = lambda t: t.view(torch.int32)
    assert d["dec1"]() == 0 and d["seg1"]() == 0, _.dal3_last_error()
    torch.cuda.synchronize()
    print(f"{name}: one wave per tile (DAL3_BCN_NO_DEC_PAIR) bitwise-equal to the first build (logits / mask of dec1, logits / mask "
          f"of seg1) = {(torch.equal(bits(d['logits1']), bits(ref['logits'])), torch.equal(d['mask1'], ref['mask']), torch.equal(bits(d['lg_seg']), bits(ref['lg_seg0'])), torch.equal(d['mk_seg'], ref['mk_seg0']))}")
    assert d["seg"]() == 0, _.dal3_last_error()
    torch.cuda.synchronize()
    seg_same = (torch.equal(bits(d["g_seg"]), bits(ref["g_seg"])), torch.equal(bits(d["lg_seg"]), bits(ref["lg_seg0"])),
                torch.equal(d["mk_seg"], ref["mk_seg0"]), torch.equal(bits(d["lg_seg0"]), bits(ref["lg_seg0"])))
    print(f"{name}: ins_seg_forward bitwise-equal to the first build without a plan (g, logits, mask, logits of its own call "
          f"without a plan) = {seg_same}")
    dl = (d["logits"] - ref["logits"]).abs().max().item() / ref["logits"].abs().max().item()
    print(f"{name}: bitwise-equal to first (g, logits, mask, box_pred) = {same}, logits rel diff {dl:.2e}")


def timed(fn, iters=5):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


KINDS = ("enc", "enc2", "dec", "dec1", "head", "head2", "seg", "seg1", "seg2", "seg0")
res = {(n, k): [] for n, _ in libs for k in KINDS}
for r in range(args.rounds):
    for k in KINDS:
        for (name, _), d in zip(libs, state):
            res[(name, k)].append(timed(d[k]))
print(f"B={B} N={N}: ms per launch, median (min, max - min) over {args.rounds} interleaved rounds")
for name, _ in libs:
    row = "  ".join(f"{k} {statistics.median(res[(name, k)]):7.3f} ({min(res[(name, k)]):7.3f}, {max(res[(name, k)]) - min(res[(name, k)]):5.3f})"
                    for k in KINDS)
    tot = sum(statistics.median(res[(name, k)]) for k in ("enc", "dec", "head"))
    print(f"{name:40s} {row}   sum {tot:7.3f}")
