#!/usr/bin/env python3
"""Diagnostic: run a -DDAL3_STAMP build of the fp32 decode kernel on the bench crops (their own per-crop term, so the tiles
take the body a step gives them) and print cycles per phase per wave.

  python tools/stamps.py variants/stamp.so [--words 16] [--B 4096] [--N 1024]

--words 8 reads a build from before the group stamps (8 words per wave, phases only). --one-wave runs the kernel with one
wave per tile (DAL3_BCN_NO_DEC_PAIR); without it a build that has the pair kernel stamps that one: per phase and per wave of
the pair, plus the ticks spent in barriers."""
import argparse, ctypes as C, importlib, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hip = importlib.import_module("3dal_pytorch_amd._hip")
synth = importlib.import_module("3dal_pytorch_amd.synth")
sm = importlib.import_module("3dal_pytorch_amd.static_model")
ap = argparse.ArgumentParser()
ap.add_argument("lib")
ap.add_argument("--words", type=int, default=16)
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--N", type=int, default=1024)
ap.add_argument("--one-wave", action="store_true")
args = ap.parse_args()
lib = C.CDLL(os.path.abspath(args.lib))
for name, (res, a) in hip.SIGNATURES.items():
    if hasattr(lib, name):
        fn = getattr(lib, name); fn.restype, fn.argtypes = res, a
B, N, W = args.B, args.N, args.words
dev = torch.device("cuda:0")
model = sm.StaticModelOneBoxEst()
model.load_state_dict({k: torch.as_tensor(v) for k, v in synth.state_dict("static_one").items()})
model = model.to(dev).eval()
pts_np = synth.static_crops(min(B, 512), N)[0]
pts = torch.from_numpy(pts_np).to(dev).repeat((B + pts_np.shape[0] - 1) // pts_np.shape[0], 1, 1)[:B].contiguous().transpose(2, 1)
arr = (hip.Layer * 10)(*[hip.layer_struct(c, b) for c, b in model.ins_seg.pairs()])
need = C.c_size_t(0)
lib.dal3_pack_weights(0, arr, 10, 0, None, C.byref(need), None)
w = torch.zeros(need.value, dtype=torch.uint8, device=dev)
st = hip.stream()
assert lib.dal3_pack_weights(0, arr, 10, 0, hip.ptr(w), C.byref(need), st) == 0
stamps = torch.zeros(2048 * 4 * 16, dtype=torch.int64, device=dev)   # (sized for 16 words whatever the build writes)
lib.dal3_debug_set_stamps.argtypes = [C.c_void_p]
assert lib.dal3_debug_set_stamps(stamps.data_ptr()) == 0
g = torch.zeros((B, 1024), device=dev)
gb = torch.empty((B, 512), device=dev)
assert lib.dal3_ins_seg_encode(hip.ptr(w), 0, 3, hip.bcn(pts), B, N, hip.ptr(g), st) == 0
assert lib.dal3_ins_seg_global_bias(hip.ptr(w), 0, hip.ptr(g), B, hip.ptr(gb), st) == 0
logits = torch.empty((B, N, 2), device=dev); mask = torch.empty((B, N), dtype=torch.uint8, device=dev)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
view = hip.bcn(pts)
if args.one_wave:
    view.flags |= hip.BCN_NO_DEC_PAIR
for i in range(3):
    if i == 2:
        ev[0].record()
    assert lib.dal3_ins_seg_decode(hip.ptr(w), 0, 3, view, B, N, hip.ptr(gb), hip.ptr(logits), hip.ptr(mask), st) == 0
ev[1].record()
torch.cuda.synchronize()
ms = ev[0].elapsed_time(ev[1])
s = stamps.cpu().numpy()[:2048 * 4 * W].reshape(-1, W)
s = s[s[:, 4] > 0]


def row(name, v):
    print(f"{name:58s} mean {v.mean():9.0f} cyc  p10 {np.percentile(v, 10):8.0f}  p90 {np.percentile(v, 90):8.0f}")


if W >= 16 and len(s) and (s[:, 15] == 1).all():          # the pair kernel: rows 2 i, 2 i + 1 are the waves of workgroup i
    print(f"pair kernel: waves sampled {len(s)}; launch {ms:.3f} ms (stamped build)")
    raw = stamps.cpu().numpy().reshape(-1, 2, 16)
    raw = raw[(raw[:, :, 4] > 0).all(axis=1)]
    for wv in (0, 1):
        t = raw[:, wv]
        print(f"-- wave {wv} of the pair")
        for name, a, b in (("prologue: points, conv1, conv2", 0, 1), ("dconv1 + dconv2 (groups, their barriers)", 1, 2),
                           ("dconv3 (two barriers, rows, list, loop)", 2, 6), ("dconv4 (the same)", 6, 3),
                           ("dconv5, its barrier, store", 3, 4), ("tile, first to last stamp", 0, 4)):
            row(name, (t[:, b] - t[:, a]).astype(np.float64))
        row("of that in barriers", t[:, 8].astype(np.float64))
        row("barriers", t[:, 9].astype(np.float64))
        row("k-steps of dconv2", t[:, 10].astype(np.float64))
    row("start of wave 1 after wave 0", (raw[:, 1, 0] - raw[:, 0, 0]).astype(np.float64))
    row("end of the later wave after the earlier", np.abs(raw[:, 1, 4] - raw[:, 0, 4]).astype(np.float64))
    tile = (raw[:, :, 4].max(axis=1) - raw[:, :, 0].min(axis=1)).astype(np.float64)
    row("pair, first to last stamp", tile)
    pairs_per_cu = B * ((N + 31) // 32) / (256 * 4)
    for ghz in (2.35, 2.42):
        print(f"at {ghz} GHz: {ms * 1e6 * ghz / pairs_per_cu:9.0f} cycles per tile of launch time (four pairs a CU), stamped pair {tile.mean():9.0f}")
    sys.exit(0)
sp = s[:, 5] > 0                                          # the compacted body stamps 5..7 too
print(f"waves sampled {len(s)}, of them in the compacted body {int(sp.sum())}; launch {ms:.3f} ms (stamped build)")


for what, t, order, names in (
        ("dense body", s[~sp], (0, 1, 2, 3, 4),
         ["prologue: points, conv1, conv2, ring start", "dconv1 + dconv2", "ReLU of dconv2", "dconv3 + dconv4", "dconv5 on the VALU, store"]),
        ("compacted body", s[sp], (0, 1, 2, 5, 6, 7, 3, 4),
         ["prologue: points, conv1, conv2, ring start", "dconv1 + dconv2 (groups)", "dconv3: producer (rows, ballots, list) and steps under it",
          "dconv3: rest of the compact loop", "dconv4: producer and steps under it", "dconv4: rest of the compact loop",
          "dconv5 on the VALU, store"])):
    if not len(t):
        continue
    print(f"-- {what}")
    for i, n in enumerate(names):
        row(n, (t[:, order[i + 1]] - t[:, order[i]]).astype(np.float64))
    tile = (t[:, 4] - t[:, 0]).astype(np.float64)
    row("tile, first to last stamp", tile)
    if W >= 16 and what == "compacted body":
        for i in range(3):
            ok = t[:, 11 + i] > 0
            steps = (t[ok, 14] >> (16 * i)) & 0xFFFF
            span = (t[ok, 11 + i] - t[ok, 8 + i]).astype(np.float64)
            row(f"dconv2 group {i}: entry to exit ({steps.mean():.1f} k-steps)", span)
            row(f"dconv2 group {i}: the same minus 512 cycles per k-step", span - 512.0 * steps)
# the turnover of a workgroup slot: launch time x clock / tiles per SIMD, minus the stamped tile (the clock is not known
# here: both ends of the range the counters give)
tiles_per_simd = B * ((N + 31) // 32) / (256 * 4)
tile = (s[:, 4] - s[:, 0]).mean()
for ghz in (2.35, 2.42):
    print(f"at {ghz} GHz: {ms * 1e6 * ghz / tiles_per_simd:9.0f} cycles per tile of launch time, stamped tile {tile:9.0f}, "
          f"turnover {ms * 1e6 * ghz / tiles_per_simd - tile:8.0f}")
