"""tests/head_screen_model.py — a CPU MODEL of the screened conv4 of the fp32 point heads (csrc/dal3_head_screen.hip; test
infrastructure, numpy/torch, in the style of tests/screen_model.py).

The head keeps of conv4's 512 x M outputs per item only the channel maxima. An item's SEED tiles (32 points; the live
tiles whose index is a multiple of the stride S, tile 0 always) are computed densely and exactly; on every other live
tile conv4 is evaluated on the fp16 MFMA (operands rounded to fp16, products summed in fp32 in an order nobody
specifies), its distance to the dense kernel's value chain32 (a k-ordered fp32 fmaf chain) is bounded by

  E(c, tile) = X * P_c + Q_c,  X = max ||x_p||_2 over the tile's 32 points,
  P_c = KAPPA ||w_c||_2 + 2^-24 sqrt(K),  Q_c = 2^-24 ||w_c||_1 + 2^-40,  KAPPA = 1.02 * 2^-10 + K * 2^-23,  K = 256

(DESIGN.md "Screened conv4 of the point heads"; dal3_misc.hip, bound_coefficients), and only the pairs with
  s16 > thr = fl(fl(G - b_c) - fl(E + 2^-22 (|G| + |b_c|))),   G = the seed tiles' exact maximum of the channel,
are recomputed exactly. (The kernel's G may be larger — other waves' and the run's own exact maxima — which only
removes candidates; the model keeps the rule of the design's table.) float64 on the fp32 operands stands in for the
exact chain; the chain's own rounding (<= K 2^-24 sum|w||x|) is part of KAPPA.
"""
import numpy as np
import torch

import bound_model
from bound_model import fold as _fold
from oracle import ref_heads as R

K = 256
KAPPA = bound_model.kappa(K)
TILE = 32
F16_GUARD = 60000.0                                       # activations above this: the tile takes the dense layer
SCR_CAP = 1024                                            # candidate entries per 32-point tile (HEAD_SCR_CAP)
STRIDE = 4                                                # DAL3_HEAD_SCR_STRIDE as shipped


def activations(sd, x, p="box_est"):
    """x (B,Cin,M) fp32 -> conv3's output x3 (B,256,M) fp32 and conv4's folded (w4 (512,256), b4 (512,))"""
    for layer, bn in (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3")):
        w, b = _fold(sd, p, layer, bn)
        x = torch.relu(torch.einsum("oc,bcn->bon", w, x) + b[None, :, None])
    w4, b4 = _fold(sd, p, "conv4", "bn4")
    return x, w4, b4


def effective_points(x, distinct):
    """x (B,M,C), distinct (B,) or None -> (the points as the kernels see them (B, Mp, C), Mp a multiple of 32: position i
    of item b holds point min(i, n_eff - 1); live (B, Mp / 32) bool: the tiles on the worklist; real (B, Mp) bool: the
    positions that are not the ragged last tile's copies of the item's last point, which the kernel never lists)"""
    B, M, _ = x.shape
    n_eff = torch.full((B,), M, dtype=torch.int64) if distinct is None else torch.as_tensor(distinct).long().clamp(1, M)
    Mp = (M + TILE - 1) // TILE * TILE
    pos = torch.minimum(torch.arange(Mp)[None, :], (n_eff - 1)[:, None])
    xe = torch.gather(x, 1, pos[:, :, None].expand(B, Mp, x.shape[2]))
    live = torch.arange(Mp // TILE)[None, :] * TILE < n_eff[:, None]
    return xe, live, torch.arange(Mp)[None, :] < n_eff[:, None]


def coefficients(w4):
    return bound_model.coefficients(w4, K)


def check(w4, b4, x3, live, real, stride=STRIDE, what="", proof=True):
    """the properties the proof gives, on one batch: x3 (B,256,Mp) fp32, live (B,tiles) bool, real (B,Mp) bool. Returns
    the report. proof=False: the report only, with the fp32 product standing in for the exact chain (the lists'
    occupancy on inputs too large for the float64 pass)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    B, _, Mp = x3.shape
    nt = Mp // TILE
    s16 = torch.einsum("oc,bcn->bon", w4.half().float(), x3.half().float())            # fp32
    exact = torch.einsum("oc,bcn->bon", w4.double(), x3.double()) if proof else torch.einsum("oc,bcn->bon", w4, x3.float())
    # E per (channel, tile) IN FP32 with the kernel's margins: X = sqrtf(max sum x^2) (1 + 2^-15); E = fmaf(X, P, Q)(1 + 2^-20)
    x = x3.float()
    ss = (x * x).sum(1).view(B, nt, TILE).amax(-1)
    X = torch.sqrt(ss) * f(1.0 + 2.0 ** -15)
    dense = (x.amax(1).view(B, nt, TILE).amax(-1) > F16_GUARD) & live                    # tiles that leave the screen for range
    P, Q = (t.float() for t in coefficients(w4))
    E = X[:, None, :] * P[None, :, None] + Q[None, :, None]                              # (B,512,tiles)
    E = E * f(2.0 ** -20) + E
    seed = live & (torch.arange(nt)[None, :] % stride == 0)
    scr = live & ~seed & ~dense                                                          # the tiles that are screened
    per_pt = lambda t: t.unsqueeze(-1).expand(*t.shape, TILE).reshape(*t.shape[:-1], Mp)
    scr_p, seed_p, live_p, dense_p = (per_pt(t)[:, None, :] for t in (scr, seed, live, dense))
    Ep = per_pt(E)

    err = torch.where(scr_p.expand_as(exact), (s16.double() - exact).abs(), torch.zeros_like(exact))
    ratio = float((err / Ep.double()).max())
    assert ratio <= 1.0 or not proof, (what, "true error / E", ratio)

    b = b4.float()[None, :, None]
    ninf = torch.full_like(exact, -np.inf)
    # G: the seed tiles' exact maximum as the dense kernel leaves it in feat: relu(fl32(max chain + b))
    top_seed = torch.where(seed_p.expand_as(exact), exact, ninf).amax(2)
    G = torch.relu((top_seed + b4.double()[None, :]).float())                              # (B,512) fp32
    Gb = G[:, :, None]
    thr = (Gb - b) - ((Gb.abs() + b.abs()) * f(2.0 ** -22) + Ep)
    cand = (s16 > thr) & scr_p & real[:, None, :]

    # the fp32 arg-max over the item's live points is a seed point, a candidate or a point of a dense tile
    arg = torch.where((live_p & real[:, None, :]).expand_as(exact), exact, ninf).argmax(2, keepdim=True)
    covered = (cand | seed_p | dense_p).expand_as(cand)
    positive = torch.where(live_p.expand_as(exact), exact, ninf).amax(2) + b4.double()[None, :] > G.double()
    ok = covered.gather(2, arg)[:, :, 0] | ~positive
    assert bool(ok.all()) or not proof, (what, "the fp32 arg-max is neither a seed point nor a candidate", int((~ok).sum()))
    # a skipped pair cannot raise the result: chain + b <= G
    skipped = scr_p.expand_as(cand) & ~cand & real[:, None, :]      # (a copy in the ragged tile equals a listed or skipped real point)
    viol = int(((exact + b.double())[skipped] > G.double()[:, :, None].expand_as(exact)[skipped]).sum())
    assert viol == 0 or not proof, (what, "a skipped pair could raise the result", viol)

    c_tile = cand.view(B, 512, nt, TILE).sum((1, 3))[scr].double()                        # candidates per screened tile
    n_live = int(live.sum())
    return {"what": what, "stride": stride, "err_over_E": ratio if proof else None, "live_tiles": n_live,
            "live_share": n_live / float(live.numel()), "seed_share": float(seed.sum()) / max(n_live, 1),
            "tiles_dense_for_range": int(dense.sum()), "screened_tiles": int(scr.sum()),
            "cand_mean": float(c_tile.mean()) if c_tile.numel() else 0.0,
            "cand_p99": float(torch.quantile(c_tile, 0.99)) if c_tile.numel() else 0.0,
            "cand_max": int(c_tile.max()) if c_tile.numel() else 0,
            "tiles_over_cap": float((c_tile > SCR_CAP).double().mean()) if c_tile.numel() else 0.0}


def run(sd, x, distinct, p="box_est", stride=STRIDE, what="", proof=True):
    """x (B,M,C) fp32 points (numpy or torch), distinct (B,) or None"""
    x = torch.as_tensor(x).float()
    xe, live, real = effective_points(x, distinct)
    x3, w4, b4 = activations(R.as_torch_sd(sd) if not torch.is_tensor(next(iter(sd.values()))) else sd, xe.transpose(2, 1), p)
    return check(w4, b4, x3, live, real, stride, what, proof)


def occupancy(sd, x, distinct, p="box_est", stride=STRIDE, chunk=64):
    """(tiles that leave the screen for range, screened tiles, screened tiles over the list's capacity) of a large batch"""
    dense = scr = over = 0
    for lo in range(0, len(x), chunk):
        d = None if distinct is None else distinct[lo:lo + chunk]
        r = run(sd, x[lo:lo + chunk], d, p, stride, proof=False)
        dense += r["tiles_dense_for_range"]
        scr += r["screened_tiles"]
        over += int(round(r["tiles_over_cap"] * r["screened_tiles"]))
    return dense, scr, over


def gpu_batch(M):
    """the smallest batch of M-point items that takes the screened route (the library's dispatch minimum, in 32-point
    tiles), plus a few items; never fewer than the special and adversarial items need"""
    import importlib
    lib = importlib.import_module("3dal_pytorch_amd._hip").lib()
    tiles = (M + TILE - 1) // TILE
    return max((int(lib.dal3_point_head_screen_min_tiles()) + tiles - 1) // tiles + 8, 48)


def gpu_case(kind, head, c_in, B, M, stride=STRIDE, seed=5):
    """The ordinary inputs of tests/test_gpu_head_screen.py: synthetic crops' points (the first M of each item), random
    counts of distinct points with the special ones in front, the points beyond an item's count copies of its first
    ones (what a real sampler delivers). Returns (state dict, x (B,M,c_in) fp32 numpy, distinct (B,) int32)."""
    from _common import synth
    rng = np.random.default_rng(seed)
    if kind == "static_one":
        pts = synth.static_crops(B, M, seed=seed)[0]
    else:
        pts = synth.dynamic_items(B, seed=seed)[0][:, :M]
    x = np.ascontiguousarray(pts[:, :, :c_in]).astype(np.float32)
    d = rng.integers(0, M + 1, size=B).astype(np.int32)
    sp = special_counts(M, stride)
    d[:len(sp)] = sp
    for b in range(B):
        k = int(min(max(d[b], 1), M))
        x[b, k:] = x[b, np.arange(M - k) % k]
    return synth.state_dict(kind, seed=23), x, d


def bench_objects(n_crops, sd, n_obj=512):
    """The bench mix of the design's table: the first n_crops bench crops, the oracle's mask with the segmentation bias
    re-centred at the mean margin; an item's distinct points are its first min(count, n_obj) positives, then copies.
    Returns (obj (B, n_obj, 3) fp32, distinct (B,) int32)."""
    from _common import synth
    pts_np, _, _ = synth.static_crops(n_crops, 1024)
    pts = torch.from_numpy(pts_np)
    lg = R.ins_seg(R.as_torch_sd(sd), pts.transpose(2, 1))
    margin = lg[:, :, 1] - lg[:, :, 0]
    mask = margin > margin.mean()
    obj = torch.zeros((n_crops, n_obj, 3))
    distinct = np.zeros(n_crops, np.int32)
    for i in range(n_crops):
        pos = torch.nonzero(mask[i]).squeeze(1)[:n_obj]
        k = len(pos)
        distinct[i] = k
        if k:
            obj[i] = pts[i][pos[torch.arange(n_obj) % k]]
    return obj, distinct


def special_counts(M, stride=STRIDE):
    """the counts of distinct points the GPU tests place in front of a batch: only seed tiles, exactly one screened tile,
    ragged last tiles, whole items, and values the library clamps"""
    return np.array([0, 1, 31, 32, 33, 32 * stride - 1, 32 * stride, 32 * stride + 1, M - 1, M], np.int32)


def adversarial(obj, distinct):
    """the adversarial items of the model and of the GPU tests, written into items 0..5 of a copy of (obj, distinct)"""
    o, d = obj.clone(), np.array(distinct, np.int32).copy()
    M = o.shape[1]
    o[0, M // 2:] = o[0, :M // 2]                          # duplicated points: exact ties
    d[0] = M
    o[1, :] = o[1, 0]                                      # all points equal (and all counted as distinct)
    d[1] = M
    d[2] = 1                                               # one live point
    o[2, 1:] = o[2, 0]
    o[3] *= 1e4                                            # coordinates of 1e4
    o[4] *= 1e-6                                           # ... and of 1e-6
    d[3] = d[4] = M
    return o, d
