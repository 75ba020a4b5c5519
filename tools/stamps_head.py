#!/usr/bin/env python3
"""Diagnostic: run a -DDAL3_STAMP build of the screened point head (point_head_screen_kernel) on the object points of the
bench crops, as tools/ab_kernels.py's `head` column does, and print s_memtime ticks per phase per tile.

  python tools/stamps_head.py variants/stamp.so [--B 4096] [--M 512]

Every persistent wave of the screened launch sums the ticks of its tiles' phases (csrc/dal3_head_screen.hip); the seed
launch is not stamped. The tick's length follows from the waves' own totals against the launch time of the same call, and
is printed: nothing here assumes a clock."""
import argparse, ctypes as C, importlib, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hip = importlib.import_module("3dal_pytorch_amd._hip")
synth = importlib.import_module("3dal_pytorch_amd.synth")
sm = importlib.import_module("3dal_pytorch_amd.static_model")
ap = argparse.ArgumentParser()
ap.add_argument("lib")
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--M", type=int, default=512)
args = ap.parse_args()
lib = C.CDLL(os.path.abspath(args.lib))
for name, (res, a) in hip.SIGNATURES.items():
    if hasattr(lib, name):
        fn = getattr(lib, name); fn.restype, fn.argtypes = res, a
B, M = args.B, args.M
dev = torch.device("cuda:0")
model = sm.StaticModelOneBoxEst()
model.load_state_dict({k: torch.as_tensor(v) for k, v in synth.state_dict("static_one").items()})
model = model.to(dev).eval()
pts_np = synth.static_crops(min(B, 512), max(M, 1024))[0]
pts = torch.from_numpy(pts_np).to(dev).repeat((B + pts_np.shape[0] - 1) // pts_np.shape[0], 1, 1)[:B]
obj = pts[:, :M, :].contiguous().transpose(2, 1)
pairs = model.box_est.pairs()
arr = (hip.Layer * len(pairs))(*[hip.layer_struct(c, b) for c, b in pairs])
need = C.c_size_t(0)
st = hip.stream()
lib.dal3_pack_weights(hip.HEAD_STATIC_BOX_EST, arr, len(pairs), 0, None, C.byref(need), None)
w = torch.zeros(need.value, dtype=torch.uint8, device=dev)
assert lib.dal3_pack_weights(hip.HEAD_STATIC_BOX_EST, arr, len(pairs), 0, hip.ptr(w), C.byref(need), st) == 0
W = 16
stamps = torch.zeros(1024 * W, dtype=torch.int64, device=dev)
lib.dal3_debug_set_head_stamps.argtypes = [C.c_void_p]
assert lib.dal3_debug_set_head_stamps(stamps.data_ptr()) == 0
ws = torch.empty(lib.dal3_point_head_workspace_bytes(B), dtype=torch.uint8, device=dev)
bp = torch.empty((B, 39), device=dev)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for i in range(3):
    if i == 2:
        stamps.zero_()
        ev[0].record()
    assert lib.dal3_point_head_forward(hip.HEAD_STATIC_BOX_EST, hip.ptr(w), 0, hip.bcn(obj), B, M, hip.ptr(bp), 39, hip.ptr(ws),
                                       ws.numel(), st) == 0, lib.dal3_last_error()
ev[1].record()
torch.cuda.synchronize()
ms = ev[0].elapsed_time(ev[1])
s = stamps.cpu().numpy().reshape(-1, W).astype(np.float64)
s = s[s[:, 8] > 0]
assert len(s), "no wave stamped: the job did not take the screened route (or the build has no -DDAL3_STAMP)"
tiles, scr = s[:, 8].sum(), s[:, 9].sum()
wave = s[:, :8].sum(1)
print(f"{B} x {M}: whole head call {ms:.3f} ms (stamped build, seed launch included); waves {len(s)}, tiles {int(tiles)}, "
      f"of them screened to the end {int(scr)}")
print(f"a wave's stamped ticks: mean {wave.mean():.0f}, p10 {np.percentile(wave, 10):.0f}, max {wave.max():.0f}")
names = ["conv1..conv3, next entry and points", "norm, pack, range test", "fp16 sweep", "list building", "recompute, first half of k",
         "recompute, second half of k", "flush, entry, turnover", "dense conv4 (range, flag, overflow)"]
per = [tiles, scr, scr, scr, scr, scr, tiles, max(tiles - scr, 1.0)]
what = ["tile", "screened tile", "screened tile", "screened tile", "screened tile", "screened tile", "tile", "dense tile"]
tot = s[:, :8].sum()
for k, n in enumerate(names):
    v = s[:, k].sum()
    print(f"{n:38s} {v / per[k]:9.1f} ticks per {what[k]:14s} {100 * v / tot:5.1f} % of the stamped ticks")
print(f"all phases: {tot / tiles:9.1f} ticks per tile")
