#!/usr/bin/env python3
"""Diagnostic: run a -DDAL3_STAMP build of the screened point head (point_head_screen_kernel, or point_head_resident_kernel
where the job takes that route) on the object points of the bench crops, as tools/ab_kernels.py's `head` column does, and
print s_memtime ticks per phase per tile.

  python tools/stamps_head.py variants/stamp.so [--B 4096] [--M 512] [--flags 64] [--mix]

Every persistent wave of the screened launch sums the ticks of its tiles' phases (csrc/dal3_head_screen.hip); the seed
launch is not stamped. On the resident route the first 1024 waves (256 items) are stamped, with two more phases: round 0's
bound sweep and the wait at its barrier; "flush" there holds the wait for the item's slowest wave. The tick's length
follows from the waves' own totals against the launch time of the same call, and is printed: nothing here assumes a clock.
--flags: DAL3_BCN_* for the call (64: the two launches). --mix: the bench mix of distinct points per item (the CPU oracle's
mask on the first 128 bench crops, tests/head_screen_model.py) through dal3_point_head_pool, instead of every point distinct.
A build with -DDAL3_SCREEN_COUNT as well prints the screen's counters of the stamped call, per round on the resident route."""
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
ap.add_argument("--flags", type=int, default=0)
ap.add_argument("--mix", action="store_true")
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
distinct = None
if args.mix:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import head_screen_model as H
    o, d = H.bench_objects(128, synth.state_dict("static_one"), n_obj=M)
    reps = (B + 127) // 128
    obj = o.repeat(reps, 1, 1)[:B].to(dev).contiguous().transpose(2, 1)
    distinct = torch.from_numpy(np.tile(d, reps)[:B].astype(np.int32)).to(dev)
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
feat = torch.empty((B, 512), device=dev)
view = hip.bcn(obj)
view.flags |= args.flags
if hasattr(lib, "dal3_point_head_route"):
    print(f"route {lib.dal3_point_head_route(hip.HEAD_STATIC_BOX_EST, B, M, args.flags)} (4: resident, 3: two launches)")
counts = (C.c_ulonglong * 72)() if hasattr(lib, "dal3_debug_head_screen_counts") else None
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for i in range(3):
    if i == 2:
        stamps.zero_()
        if counts is not None:
            torch.cuda.synchronize()
            lib.dal3_debug_head_screen_counts(counts, 1)
        ev[0].record()
    if distinct is not None:
        rc = lib.dal3_point_head_pool(hip.HEAD_STATIC_BOX_EST, hip.ptr(w), 0, view, B, M, hip.ptr(distinct), hip.ptr(feat), hip.ptr(ws),
                                      ws.numel(), st)
    else:
        rc = lib.dal3_point_head_forward(hip.HEAD_STATIC_BOX_EST, hip.ptr(w), 0, view, B, M, hip.ptr(bp), 39, hip.ptr(ws), ws.numel(), st)
    assert rc == 0, lib.dal3_last_error()
ev[1].record()
torch.cuda.synchronize()
ms = ev[0].elapsed_time(ev[1])
s = stamps.cpu().numpy().reshape(-1, W).astype(np.float64)
s = s[s[:, 8] > 0]
assert len(s), "no wave stamped: the job did not take the screened route (or the build has no -DDAL3_STAMP)"
tiles, scr = s[:, 8].sum(), s[:, 9].sum()
resident = bool(s[:, 10:12].sum() > 0)
wave = s[:, :8].sum(1) + s[:, 10:12].sum(1)
print(f"{B} x {M}: whole head call {ms:.3f} ms (stamped build, seed launch included); waves {len(s)}, tiles {int(tiles)}, "
      f"of them screened to the end {int(scr)}")
print(f"a wave's stamped ticks: mean {wave.mean():.0f}, p10 {np.percentile(wave, 10):.0f}, max {wave.max():.0f}")
names = ["conv1..conv3, next entry and points", "norm, pack, range test", "fp16 sweep", "list building", "recompute, first half of k",
         "recompute, second half of k", "flush, entry, turnover", "dense conv4 (range, flag, overflow)"]
per = [tiles, scr, scr, scr, scr, scr, tiles, max(tiles - scr, 1.0)]
what = ["tile", "screened tile", "screened tile", "screened tile", "screened tile", "screened tile", "tile", "dense tile"]
cols = list(range(8))
if resident:
    names[6] = "wait for the item's last wave, flush"
    names += ["round 0: bound sweep", "round 0: wait at the barrier"]
    per += [tiles, tiles]
    what += ["tile", "tile"]
    cols += [10, 11]
tot = s[:, cols].sum()
for k, n in zip(cols, names):
    v = s[:, k].sum()
    i = cols.index(k)
    print(f"{n:38s} {v / per[i]:9.1f} ticks per {what[i]:14s} {100 * v / tot:5.1f} % of the stamped ticks")
print(f"all phases: {tot / tiles:9.1f} ticks per tile")
if counts is not None:
    torch.cuda.synchronize()
    lib.dal3_debug_head_screen_counts(counts, 0)
    c = [int(v) for v in counts]
    print(f"counters: tiles {c[0]}, dense for range or flag {c[1]}, dense for list overflow {c[2]}, candidates {c[3]} = "
          f"{c[3] / max(c[0] - c[1], 1):.1f} per screened tile, recompute rounds {c[4]}")
    if sum(c[40:72]):
        print("candidates per screened tile by round: " + " / ".join(f"{c[8 + r] / c[40 + r]:.1f}" for r in range(32) if c[40 + r]))
        print("screened tiles by round: " + " / ".join(str(c[40 + r]) for r in range(32) if c[40 + r]))
