"""The float64 truth of the sparse 3-D middle (3dal_pytorch_amd/sparse.py; dal3_sp_* of include/dal3.h) in two formulations
that share nothing but the walk over the layers:

  `Dense`     torch.nn.functional.conv3d on the densified input with the weight permuted (4, 3, 0, 1, 2), and an explicit
              active mask carried through the levels (a submanifold layer keeps it, a SparseConv3d dilates it through the
              window); with dtype float32 the same code is the torch-CPU fp32 yardstick of the GPU tests;
  `Rulebook`  the gather the kernels use: sorted 32-bit keys, output sites as the unique candidate keys in ascending order,
              tap-major neighbour tables, a sum over the present taps. Its integers (indices, counts, tables) are what the
              GPU bookkeeping is compared with, exactly.

spconv cannot be imported here: the definition is the issue's (spconv 1.x: weight (kD, kH, kW, c_in, c_out), a
cross-correlation, out = floor((in + 2 pad - k) / s) + 1), and that the two formulations agree to 1e-12 of the tensor's
maximum on the test grids is what tests/test_sparse_cpu.py pins. `fold` restates the packing's arithmetic bit for bit.
`fault=` plants one wrong reading of the definition at a time. The measures are pillars_ref.judge's on (cells, channels)."""
import numpy as np
import torch
from torch.nn import functional as F

import fold_ref
import pillars_ref as P
import rpn_ref as R

synth = P.synth
SEED = 20241019
EPS = 1e-3
MEASURES, FLOOR = P.MEASURES, P.FLOOR
# name, c_out, kernel, stride, padding of the five stems; two SparseBasicBlocks of c_out follow each but the last
STEMS = (("conv_input", 16, (3, 3, 3), (1, 1, 1), (1, 1, 1)), ("conv2", 32, (3, 3, 3), (2, 2, 2), (1, 1, 1)),
         ("conv3", 64, (3, 3, 3), (2, 2, 2), (1, 1, 1)), ("conv4", 128, (3, 3, 3), (2, 2, 2), (0, 1, 1)),
         ("extra_conv", 128, (3, 1, 1), (2, 1, 1), (0, 0, 0)))
LEVELS = ("conv1", "conv2", "conv3", "conv4")
FAULTS = ("taps_flipped", "conv4_padded_111", "eps_1e-5", "bias_leaks", "residual_dropped", "interleave_dC", "subm_dilates")
GRID = (41, 37, 45)                             # D 41 -> 21 -> 11 -> 5 -> 2, H 37 -> 19 -> 10 -> 5, W 45 -> 23 -> 12 -> 6

# The GPU tests' bars: multiples of the yardstick (the torch-CPU fp32 masked dense evaluation's own error against the
# float64 truth on the same input), by the rule written beside pillars_ref.BARS. Set before any MI355X run, on that
# rule's reasoning: kernel and yardstick are fp32 evaluations of the same chain of dot products of at most 27 x 128 terms;
# the kernel rounds every folded weight once more (a term's rms error grows by at most sqrt(2)) and sums in another
# order (the same bound), and the per-channel measures are maxima over up to 128 channels of a few hundred sites, which
# move by about 2 x between two equally good evaluations: 4 = sqrt(2) x 2, rounded up. The first run on an MI355X
# (profiles/sparse_measured.json, DAL3_SPARSE_RECORD over tests/test_gpu_sparse.py and tests/test_gpu_voxelnet.py in one
# session: 61 rows — 45 single layers, the backbone's BEV map and four levels for 5 and 6 input features, the same with
# a NaN and an Inf, the row with bad coordinates) recorded at worst tensor 2.03 and chan_rms 1.97 (both
# layer/128-128/canvas) and chan_max 1.39 (layer/64-64/canvas): x 2 gives 4.07 (the bar stays at 4 = 1.97 x the worst: a bar
# does not go up), 3.9 -> 4 and 2.8 -> 3. The whole backbone stayed between 0.27 and 0.9. The smallest planted-fault
# ratio of tests/test_sparse_cpu.py is 2.6e2 (bias_leaks, tensor): every bar is under a tenth of it.
BARS = {"tensor": 4.0, "chan_rms": 4.0, "chan_max": 3.0}


def out_shape(shape, kernel, stride, padding):
    return tuple((int(n) + 2 * p - k) // s + 1 for n, k, s, p in zip(shape, kernel, stride, padding))


# ------------------------------------------------------------------------------------- seeded inputs and weights
def clustered(tag, shape, n_clusters=2, per_cluster=160, sigma=2.5):
    """one sample's voxels around a few centres -> (n, 3) int32 [z, y, x], unique, in a seeded scrambled order. Uniform
    occupancy would saturate the coarse levels: 2 % of 41 x 37 x 45 fills all of the 2 x 5 x 6 output."""
    D, H, W = shape
    ext = np.asarray([D, H, W], np.float64)
    centres = synth.uniform(SEED, f"{tag}/centres", (n_clusters, 3), 0.15, 0.6) * ext
    pts = centres[:, None, :] + synth.normal(SEED, f"{tag}/pts", (n_clusters, per_cluster, 3), 0.0, sigma)
    c = np.clip(np.floor(pts.reshape(-1, 3)), 0, ext - 1).astype(np.int64)
    key = np.unique((c[:, 0] * H + c[:, 1]) * W + c[:, 2])
    order = np.argsort(synth.uniform(SEED, f"{tag}/order", (key.size,)), kind="stable")
    key = key[order]
    return np.stack([key // (H * W), (key // W) % H, key % W], 1).astype(np.int32)


def batch(samples):
    """[(n_b, 3) per sample] -> (n, 4) int32 [b, z, y, x]"""
    rows = [np.concatenate([np.full((len(s), 1), b, np.int32), np.asarray(s, np.int32).reshape(-1, 3)], 1) for b, s in enumerate(samples)]
    return np.concatenate(rows, 0) if rows else np.zeros((0, 4), np.int32)


def backbone_case(c_in=5, shape=GRID):
    """B = 3: a clustered sample, an empty one, and two voxels at opposite corners of the 40-cell-deep voxel grid"""
    D, H, W = shape
    idx = batch([clustered("bb/0", (D - 1, H, W)), np.zeros((0, 3)), [[0, 0, 0], [D - 2, H - 1, W - 1]]])
    feats = synth.uniform(SEED, f"bb/feats/{c_in}", (idx.shape[0], c_in), 0.0, 2.0).astype(np.float32)
    return feats, idx, 3, shape


def layer_weights(tag, kernel, c_in, c_out, bias, bn):
    """seeded parameters of one layer -> (w (kD, kH, kW, c_in, c_out), bias or None, (g, beta, mean, var) or None). The
    fan-in counts a third of the taps: most neighbours of a sparse site are absent"""
    taps = int(np.prod(kernel))
    w = R._w(tag, (c_out, c_in, *kernel), c_in * max(taps // 3, 1))
    w = np.ascontiguousarray(w.transpose(2, 3, 4, 1, 0))
    b = synth.uniform(SEED, tag + "/bias", (c_out,), -0.5, 0.5).astype(np.float32) if bias else None
    sd = {}
    if bn:
        R._bn(sd, "", tag, c_out)
    return w, b, (R.bn_of(sd, "") if bn else None)


def backbone_weights(c_in=5, tag="scn"):
    """a reference-keyed state_dict of SpMiddleResNetFHD(num_input_features=c_in)"""
    sd, cin = {}, c_in

    def put(p_conv, p_bn, t, kernel, ci, co, bias):
        w, b, bn = layer_weights(t, kernel, ci, co, bias, True)
        sd[p_conv + "weight"] = w
        if bias:
            sd[p_conv + "bias"] = b
        for k, v in zip(("weight", "bias", "running_mean", "running_var"), bn):
            sd[p_bn + k] = v
        sd[p_bn + "num_batches_tracked"] = np.asarray(7, np.int64)

    for name, c, kernel, _, _ in STEMS:
        put(f"{name}.0.", f"{name}.1.", f"{tag}/{c_in}/{name}", kernel, cin, c, False)
        if name != "extra_conv":
            seq = "conv1" if name == "conv_input" else name
            for j in ((0, 1) if name == "conv_input" else (3, 4)):
                for k in (1, 2):
                    put(f"{seq}.{j}.conv{k}.", f"{seq}.{j}.bn{k}.", f"{tag}/{c_in}/{seq}/{j}/{k}", (3, 3, 3), c, c, True)
        cin = c
    return sd


def fold(w, bias, bn, eps=EPS):
    """fold_ref.fold with spconv's (kD, kH, kW, c_in, c_out) weight"""
    return fold_ref.fold(w, bias, bn, eps, -1)


# ------------------------------------------------------------------------------------- the rulebook (integers)
def keys_of(idx, B, shape):
    """(n) int64 keys, -1 for rows outside the grid or the batch"""
    D, H, W = shape
    i = np.asarray(idx, np.int64).reshape(-1, 4)
    ok = (i[:, 0] >= 0) & (i[:, 0] < B) & (i[:, 1] >= 0) & (i[:, 1] < D) & (i[:, 2] >= 0) & (i[:, 2] < H) & (i[:, 3] >= 0) & (i[:, 3] < W)
    return np.where(ok, ((i[:, 0] * D + i[:, 1]) * H + i[:, 2]) * W + i[:, 3], -1)


def unkey(key, shape):
    D, H, W = shape
    key = np.asarray(key, np.int64)
    return np.stack([key // (D * H * W), (key // (H * W)) % D, (key // W) % H, key % W], 1).astype(np.int32)


def sort_sites(idx, B, shape, capacity=None):
    """-> (sorted_key, sorted_pos) int32 (capacity): a stable sort; rows that are no site carry B * D * H * W at the end"""
    none = B * int(np.prod(shape))
    k = keys_of(idx, B, shape)
    k = np.where(k < 0, none, k)
    if capacity is not None:
        k = np.concatenate([k, np.full(capacity - k.size, none, np.int64)])
    order = np.argsort(k, kind="stable")
    return k[order].astype(np.int32), order.astype(np.int32)


def downsample(idx, B, shape, kernel, stride, padding):
    """the active output sites of a SparseConv3d in ascending key order -> ((n_out, 4) int32, out shape)"""
    osh = out_shape(shape, kernel, stride, padding)
    i = np.asarray(idx, np.int64).reshape(-1, 4)
    i = i[keys_of(i, B, shape) >= 0]
    found = []
    for kz in range(kernel[0]):
        for ky in range(kernel[1]):
            for kx in range(kernel[2]):
                num = i[:, 1:] + np.asarray(padding) - np.asarray([kz, ky, kx])     # = o * stride
                o = num // np.asarray(stride)
                ok = np.all((num % np.asarray(stride) == 0) & (o >= 0) & (o < np.asarray(osh)), 1)
                found.append(keys_of(np.concatenate([i[ok, :1], o[ok]], 1), B, osh))
    key = np.unique(np.concatenate(found)) if found else np.zeros(0, np.int64)
    return unkey(key, osh), osh


def table(out_idx, in_idx, B, in_shape, osh, kernel, stride, padding):
    """(taps, n_out) int32, tap = (kz * kH + ky) * kW + kx: the input row under each tap, -1 for none. A bad output row
    (outside its grid) has none."""
    ik = keys_of(in_idx, B, in_shape)
    where = {int(k): r for r, k in enumerate(ik) if k >= 0}
    o = np.asarray(out_idx, np.int64).reshape(-1, 4)
    good = keys_of(o, B, osh) >= 0
    t = np.full((int(np.prod(kernel)), o.shape[0]), -1, np.int32)
    tap = 0
    for kz in range(kernel[0]):
        for ky in range(kernel[1]):
            for kx in range(kernel[2]):
                c = o[:, 1:] * np.asarray(stride) - np.asarray(padding) + np.asarray([kz, ky, kx])
                k = keys_of(np.concatenate([o[:, :1], c], 1), B, in_shape)
                t[tap] = [where.get(int(v), -1) if (v >= 0 and g) else -1 for v, g in zip(k, good)]
                tap += 1
    return t


def table_sorted(out_idx, in_idx, B, in_shape, osh, kernel, stride, padding):
    """`table` without the dict: one np.searchsorted per tap over the valid input keys in a stable ascending order. The
    same signature and the same result (of input rows that share a key the last one answers, as the dict's later entry
    replaces the earlier one; -1 for a bad output row and for a tap outside the input grid): what a level of tens of
    thousands of sites is compared with."""
    ik = keys_of(in_idx, B, in_shape)
    rows = np.nonzero(ik >= 0)[0]
    rows = rows[np.argsort(ik[rows], kind="stable")]
    sk = ik[rows]
    o = np.asarray(out_idx, np.int64).reshape(-1, 4)
    good = keys_of(o, B, osh) >= 0
    t = np.full((int(np.prod(kernel)), o.shape[0]), -1, np.int32)
    tap = 0
    for kz in range(kernel[0]):
        for ky in range(kernel[1]):
            for kx in range(kernel[2]):
                c = o[:, 1:] * np.asarray(stride) - np.asarray(padding) + np.asarray([kz, ky, kx])
                k = keys_of(np.concatenate([o[:, :1], c], 1), B, in_shape)
                if sk.size:
                    at = np.searchsorted(sk, k, side="right") - 1
                    hit = good & (k >= 0) & (at >= 0) & (sk[np.maximum(at, 0)] == k)
                    t[tap, hit] = rows[at[hit]]
                tap += 1
    return t


# ------------------------------------------------------------------------------------- the two formulations
class Rulebook:
    """x = (features (n, C) of `dtype`, indices (n, 4), shape); `record` holds the integers by level. dtype float32 is the
    same gather evaluated in fp32: the yardstick on a grid too large for the dense formulation. table: `table` or its
    vectorised twin `table_sorted`."""

    def __init__(self, B, fault=None, dtype=np.float64, table=table):
        self.B, self.fault, self.cache, self.record, self.dtype, self.table = B, fault, {}, {}, dtype, table

    def start(self, feats, idx, shape):
        f = np.asarray(feats, self.dtype).copy()
        f[keys_of(idx, self.B, shape) < 0] = 0.0
        return f, np.asarray(idx, np.int32), tuple(shape)

    def conv(self, x, w, kernel, stride, padding, subm, key):
        f, idx, shape = x
        w = np.asarray(w, self.dtype)
        if self.fault == "taps_flipped":
            w = w[::-1, ::-1, ::-1]
        if subm:
            if key not in self.cache:
                self.cache[key] = self.table(idx, idx, self.B, shape, shape, (3, 3, 3), (1, 1, 1), (1, 1, 1))
            t, oidx, osh = self.cache[key], idx, shape
        else:
            oidx, osh = downsample(idx, self.B, shape, kernel, stride, padding)
            t = self.table(oidx, idx, self.B, shape, osh, kernel, stride, padding)
        self.record[key] = dict(indices=oidx, shape=osh, table=t)
        w = w.reshape(-1, w.shape[3], w.shape[4])
        y = np.zeros((oidx.shape[0], w.shape[2]), self.dtype)
        for tap in range(t.shape[0]):
            has = t[tap] >= 0
            if has.any():
                y[has] += f[t[tap][has]] @ w[tap]
        self.valid = (keys_of(oidx, self.B, osh) >= 0)[:, None]
        return y, oidx, osh

    def post(self, x, fn):
        y, idx, shape = x
        return np.where(self.valid, fn(y, lambda v: np.asarray(v, self.dtype)[None, :]), self.dtype(0)), idx, shape

    def feats(self, x):
        return x[0]

    def dense(self, x):
        f, idx, (D, H, W) = x
        out = np.zeros((self.B, D, H, W, f.shape[1]))
        ok = keys_of(idx, self.B, (D, H, W)) >= 0
        out[idx[ok, 0], idx[ok, 1], idx[ok, 2], idx[ok, 3]] = f[ok]
        return out.transpose(0, 4, 1, 2, 3)


class Dense:
    """x = (map (B, C, D, H, W), mask (B, 1, D, H, W) bool), torch CPU tensors of `dtype`"""

    def __init__(self, B, dtype=torch.float64, fault=None):
        self.B, self.dtype, self.fault, self.record = B, dtype, fault, {}

    def start(self, feats, idx, shape):
        D, H, W = shape
        ok = keys_of(idx, self.B, shape) >= 0
        i = torch.as_tensor(np.asarray(idx, np.int64)[ok])
        x = torch.zeros((self.B, D, H, W, feats.shape[1]), dtype=self.dtype)
        x[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = torch.as_tensor(np.asarray(feats)[ok]).to(self.dtype)
        m = torch.zeros((self.B, D, H, W), dtype=torch.bool)
        m[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = True
        return x.permute(0, 4, 1, 2, 3).contiguous(), m[:, None]

    def conv(self, x, w, kernel, stride, padding, subm, key):
        x, m = x
        wt = torch.as_tensor(np.ascontiguousarray(w)).to(self.dtype).permute(4, 3, 0, 1, 2)
        if self.fault == "taps_flipped":
            wt = wt.flip(2, 3, 4)
        if subm:
            kernel, stride, padding = (3, 3, 3), (1, 1, 1), (1, 1, 1)
        # an inactive cell may hold a NaN only where the mask later removes it; the sum itself must not see it
        y = F.conv3d(torch.where(m, x, torch.zeros((), dtype=self.dtype)), wt.contiguous(), stride=stride, padding=padding)
        if subm and self.fault != "subm_dilates":
            mo = m
        else:
            mo = F.conv3d(m.to(torch.float64), torch.ones((1, 1, *kernel), dtype=torch.float64), stride=stride, padding=padding) > 0
        self.record[key] = mo[:, 0].numpy()
        return y, mo

    def post(self, x, fn):
        y, m = x
        y = fn(y, lambda v: torch.as_tensor(np.asarray(v)).to(self.dtype).reshape(1, -1, 1, 1, 1))
        return (y if self.fault == "bias_leaks" else torch.where(m, y, torch.zeros((), dtype=self.dtype))), m

    def feats(self, x):
        return x[0]

    def dense(self, x):
        return x[0].numpy()


def _post(be, y, bias, bn, eps, relu, residual=None):
    """bias, eval-mode BatchNorm from the unfolded parameters, residual, ReLU, on the active sites"""
    xp = torch if isinstance(be, Dense) else np

    def fn(v, ch):
        if bias is not None:
            v = v + ch(bias)
        if bn is not None:
            g, beta, mean, var = bn
            v = (v - ch(mean)) / xp.sqrt(ch(var) + eps) * ch(g) + ch(beta)
        if residual is not None:
            v = v + residual
        if relu:
            v = torch.relu(v) if xp is torch else np.where(v < 0, 0.0, v)      # a NaN stays
        return v

    return be.post(y, fn)


def layer(be, feats, idx, shape, w, bias, bn, kernel, stride, padding, subm, relu, residual=False, eps=EPS):
    """one layer from the unfolded parameters -> the dense output (B, c_out, D', H', W') as a NumPy array. residual: add the
    input (a submanifold layer of equal widths)"""
    x = be.start(feats, idx, shape)
    y = be.conv(x, w, kernel, stride, padding, subm, "layer")
    return np.asarray(be.dense(_post(be, y, bias, bn, eps, relu, be.feats(x) if residual else None)))


def layer_rows(be, feats, idx, shape, w, bias, bn, kernel, stride, padding, subm, relu, eps=EPS):
    """`layer` on a Rulebook without the dense map, for a grid no dense array can hold -> (rows (n_out, c_out), output
    indices (n_out, 4), output shape): a submanifold layer's rows in the input's order, a strided one's in key order"""
    x = be.start(feats, idx, shape)
    y, oidx, osh = _post(be, be.conv(x, w, kernel, stride, padding, subm, "layer"), bias, bn, eps, relu)
    return y, oidx, osh


def backbone(be, sd, feats, idx, shape):
    """SpMiddleResNetFHD.forward from the unfolded parameters -> {"bev": (B, 256, H', W'), "conv1" .. "conv4": dense
    (B, C, D, H, W)} as NumPy arrays; with a Rulebook its `record` then holds every level's integers"""
    fault = be.fault
    eps = 1e-5 if fault == "eps_1e-5" else EPS
    x = be.start(feats, idx, shape)
    out, res = {}, 0

    def bn_of(p):
        return R.bn_of(sd, p)

    for name, c, kernel, stride, padding in STEMS:
        if name == "conv4" and fault == "conv4_padded_111":
            padding = (1, 1, 1)
        subm = name == "conv_input"
        y = be.conv(x, sd[f"{name}.0.weight"], kernel, stride, padding, subm, "res0" if subm else name)
        x = _post(be, y, None, bn_of(f"{name}.1."), eps, True)
        if name == "extra_conv":
            break
        seq = "conv1" if subm else name
        key = f"res{res}"
        for j in ((0, 1) if subm else (3, 4)):
            p = f"{seq}.{j}."
            y = be.conv(x, sd[p + "conv1.weight"], None, None, None, True, key)
            h = _post(be, y, sd[p + "conv1.bias"], bn_of(p + "bn1."), eps, True)
            y = be.conv(h, sd[p + "conv2.weight"], None, None, None, True, key)
            x = _post(be, y, sd[p + "conv2.bias"], bn_of(p + "bn2."), eps, True,
                      None if fault == "residual_dropped" else be.feats(x))
        out[seq] = np.asarray(be.dense(x))
        res += 1
    d = np.asarray(be.dense(x))                 # (B, C, D, H, W)
    B, C, D, H, W = d.shape
    if fault == "interleave_dC":
        d = d.transpose(0, 2, 1, 3, 4)
    out["bev"] = np.ascontiguousarray(d).reshape(B, C * D, H, W)
    return out


def rows_of(y):
    """(B, C, ...) -> (cells, C): the (rows, channels) layout judge takes"""
    y = np.asarray(y)
    return np.ascontiguousarray(np.moveaxis(y, 1, -1).reshape(-1, y.shape[1]))


def judge(got, truth):
    return P.judge(rows_of(got), rows_of(truth))


def ratios(got, f32, truth):
    return P.ratios(rows_of(got), rows_of(f32), rows_of(truth))


def finite_part(got, truth):
    """the non-finite sets must be equal; -> (got, truth) with those entries zeroed, for the measures"""
    got, truth = np.asarray(got), np.asarray(truth)
    bad = ~np.isfinite(truth)
    assert np.array_equal(~np.isfinite(got), bad), "the non-finite set of the output differs from the truth's"
    return np.where(bad, 0, got), np.where(bad, 0, truth)
