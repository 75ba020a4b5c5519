"""The float64 truth of the TRAIN-mode sparse 3-D middle (sparse.py's train_forward; dal3_sp_table_transposed and
dal3_sp_wgrad of include/dal3.h) in two differentiable formulations that share nothing but the walk over the layers:

  `DenseT`  sparse_ref's masked dense conv3d on torch tensors under torch.autograd; BatchNorm takes its statistics over
            the active cells only. With dtype float32 the same code is the torch-CPU fp32 yardstick of the GPU tests.
  `RuleT`   the rulebook gather on rows, each convolution a torch.autograd.Function whose backward is written out: the
            data gradient gathered through the INVERSE table (a submanifold layer: its own table with the taps mirrored; a
            SparseConv3d: `inverse_table`, the formula dal3_sp_table_transposed implements) and the weight and bias
            gradients as explicit sums over the present (tap, site) pairs. BatchNorm over the rows.

Outputs, every parameter's gradient under a seeded cotangent and the updated running statistics of the two must agree to
1e-12 of each tensor's maximum (tests/test_sparse_train_cpu.py). `fault=` plants one wrong reading at a time in `RuleT`.
The measures are pillars_ref.judge's: a weight gradient is judged as (taps * c_in, c_out) rows, a vector as one channel
of C rows (`as_rows`)."""
import numpy as np
import torch
from torch.nn import functional as F

import sparse_ref as S

synth, SEED, EPS, MEASURES = S.synth, S.SEED, S.EPS, S.MEASURES
MOMENTUM = 0.01                                 # det3d's norm_cfg for BN1d
PAD = 37                                        # the dead rows behind the count that the capacity faults see
FAULTS = ("subm_taps_not_mirrored", "wgrad_counts_dead_rows", "bn_over_capacity", "bias_grad_dropped", "running_var_biased")
TRAIN_GRID = (25, 29, 33)                       # D 25 -> 13 -> 7 -> 3 -> 1, H 29 -> 15 -> 8 -> 4, W 33 -> 17 -> 9 -> 5
TRAIN_SITES = (540, 567, 212, 78, 28)           # the input, conv2, conv3, conv4 and extra_conv levels of train_case()

# The GPU tests' bars (tests/test_gpu_sparse_train.py): multiples of the yardstick, the torch-CPU fp32 `DenseT`'s own error
# against the float64 truth on the same input, by the rule written beside pillars_ref.BARS: the worst ratio recorded on an
# MI355X x at most 2, one significant digit, under a tenth of the smallest planted-fault ratio of
# tests/test_sparse_train_cpu.py; a bar comes down or stays, it does not go up. Before the first run they stood at the
# forward's 4 / 4 / 3 doubled, 8 / 8 / 6, on reasoning: a gradient is the same kind of fp32 chain of dot products as the
# forward (dgrad: at most 27 x 128 terms, the bars of sparse_ref), but wgrad contracts over the sites in slices that are
# then added (one more summation order), and a few hundred sites make short sums whose maxima move by about 2 x between
# two equally good evaluations. The first run (profiles/sparse_train_measured.json, DAL3_SPARSE_TRAIN_RECORD over the whole
# of tests/test_gpu_sparse_train.py: 332 rows: 24 single layers and the even-depth one with y, dx, dW, db, the K-slice
# seam, a block, the backbone's outputs, 63 gradients and 42 running statistics, the same through first_stage_loss)
# recorded at worst tensor 3.23 (layer/16-32/subm/dW), chan_rms 2.37 (layer/16-32/subm/db) and chan_max 3.23
# (layer/16-16/k311s211/dW); the block, the whole backbone and first_stage_loss stayed under 1.4. x 2 gives 6.5 -> 6, 4.7 -> 4 and 6.5 -> 6. The smallest
# planted-fault ratio is 2.1e4 (running_var_biased, tensor): every bar is far under a tenth of it.
BARS = {"tensor": 6.0, "chan_rms": 4.0, "chan_max": 6.0}


def cotangent(tag, shape):
    return synth.uniform(SEED, f"cot/{tag}", tuple(shape), -1.0, 1.0)


def train_case(c_in=5):
    """B = 4 on TRAIN_GRID: two clustered samples, an empty one, two voxels at opposite corners of the voxel grid"""
    D, H, W = TRAIN_GRID
    idx = S.batch([S.clustered("tr/0", (D - 1, H, W), 3, 120, 2.2), S.clustered("tr/1", (D - 1, H, W), 2, 120, 2.2), np.zeros((0, 3)),
                   [[0, 0, 0], [D - 2, H - 1, W - 1]]])
    feats = synth.uniform(SEED, f"tr/feats/{c_in}", (idx.shape[0], c_in), 0.0, 2.0).astype(np.float32)
    return feats, idx, 4, TRAIN_GRID


# ------------------------------------------------------------------------------------- the inverse tables
def inverse_brute(table, n_in):
    """(taps, n_in): inv[k][table[k][i]] = i, read off the forward table"""
    inv = np.full((table.shape[0], n_in), -1, np.int32)
    for k in range(table.shape[0]):
        has = table[k] >= 0
        inv[k][table[k][has]] = np.nonzero(has)[0]
    return inv


def inverse_subm(table):
    """a submanifold kernel-3 layer: the forward table with the taps mirrored"""
    return table[::-1].copy()


def inverse_table(in_idx, out_idx, B, in_shape, osh, kernel, stride, padding):
    """a SparseConv3d: for input site j and tap k the output site o = (j + padding - k) / stride, when the division is exact
    on every axis and o is an active site of the output grid; out_idx: the output sites in ascending key order"""
    keys = S.keys_of(out_idx, B, osh)
    i = np.asarray(in_idx, np.int64).reshape(-1, 4)
    good = S.keys_of(i, B, in_shape) >= 0
    inv = np.full((int(np.prod(kernel)), i.shape[0]), -1, np.int32)
    tap = 0
    for kz in range(kernel[0]):
        for ky in range(kernel[1]):
            for kx in range(kernel[2]):
                num = i[:, 1:] + np.asarray(padding) - np.asarray([kz, ky, kx])
                o = num // np.asarray(stride)
                ok = good & np.all((num >= 0) & (num % np.asarray(stride) == 0) & (o < np.asarray(osh)), 1)
                k = S.keys_of(np.concatenate([i[:, :1], o], 1), B, osh)
                at = np.searchsorted(keys, k)
                hit = ok & (at < keys.size) & (keys[np.minimum(at, max(keys.size - 1, 0))] == k) if keys.size else np.zeros_like(ok)
                inv[tap, hit] = at[hit]
                tap += 1
    return inv


# ------------------------------------------------------------------------------------- the two formulations
class DenseT:
    """x = (map (B, C, D, H, W), mask (B, 1, D, H, W) bool, rows' indices or None), torch CPU tensors of `dtype`"""

    def __init__(self, B, dtype=torch.float64):
        self.B, self.dtype, self.fault = B, dtype, None

    def start(self, feats, idx, shape):
        D, H, W = shape
        ok = S.keys_of(idx, self.B, shape) >= 0
        i = torch.as_tensor(np.asarray(idx, np.int64)[ok])
        x = torch.zeros((self.B, D, H, W, feats.shape[1]), dtype=self.dtype).index_put((i[:, 0], i[:, 1], i[:, 2], i[:, 3]), feats[torch.as_tensor(ok)])
        m = torch.zeros((self.B, D, H, W), dtype=torch.bool)
        m[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = True
        return x.permute(0, 4, 1, 2, 3), m[:, None]

    def _zero(self):
        return torch.zeros((), dtype=self.dtype)

    def conv(self, x, w, b, kernel, stride, padding, subm, key):
        x, m = x
        if subm:
            kernel, stride, padding = (3, 3, 3), (1, 1, 1), (1, 1, 1)
        y = F.conv3d(torch.where(m, x, self._zero()), w.permute(4, 3, 0, 1, 2), stride=stride, padding=padding)
        mo = m if subm else F.conv3d(m.to(torch.float64), torch.ones((1, 1, *kernel), dtype=torch.float64), stride=stride, padding=padding) > 0
        if b is not None:
            y = y + b.reshape(1, -1, 1, 1, 1)
        return torch.where(mo, y, self._zero()), mo

    def bn(self, x, g, beta, mean, var, train):
        """-> (normalised x, the batch mean and UNBIASED variance or None)"""
        y, m = x
        ch = lambda v: v.reshape(1, -1, 1, 1, 1)
        if not train:
            return (torch.where(m, (y - ch(mean)) / torch.sqrt(ch(var) + EPS) * ch(g) + ch(beta), self._zero()), m), None
        cnt = m.sum().to(self.dtype)
        mu = y.sum((0, 2, 3, 4)) / cnt
        d = torch.where(m, y - ch(mu), self._zero())
        v = (d * d).sum((0, 2, 3, 4)) / cnt
        out = torch.where(m, d / torch.sqrt(ch(v) + EPS) * ch(g) + ch(beta), self._zero())
        return (out, m), (mu.detach(), (v * cnt / (cnt - 1)).detach())

    def act(self, x, residual=None):
        y, m = x
        return torch.where(m, torch.relu(y if residual is None else y + residual[0]), self._zero()), m

    def dense(self, x):
        return x[0]


class _RuleConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, w, b, table, inv, subm, fault):
        wk = w.reshape(-1, w.shape[3], w.shape[4])
        y = torch.zeros((table.shape[1], wk.shape[2]), dtype=f.dtype)
        for tap in range(table.shape[0]):
            has = torch.as_tensor(table[tap] >= 0)
            if has.any():
                y[has] += f[torch.as_tensor(table[tap].astype(np.int64))[has]] @ wk[tap]
        if b is not None:
            y = y + b
        ctx.save_for_backward(f, w)
        ctx.misc = (table, inv, subm, fault, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        f, w = ctx.saved_tensors
        table, inv, subm, fault, has_bias = ctx.misc
        wk = w.reshape(-1, w.shape[3], w.shape[4])
        taps = table.shape[0]
        # dgrad: dx[j] = sum_k dy[inv[k][j]] W[k]^T; a submanifold layer runs it on the forward table with flipped taps
        dx = torch.zeros_like(f)
        for k in range(taps):
            if subm:
                rows, wt = table[k], wk[k if fault == "subm_taps_not_mirrored" else taps - 1 - k]
            else:
                rows, wt = inv[k], wk[k]
            has = torch.as_tensor(rows >= 0)
            if has.any():
                dx[has] += dy[torch.as_tensor(rows.astype(np.int64))[has]] @ wt.T
        # wgrad: dW[k] = sum over the present pairs of x[table[k][i]]^T dy[i]; db = sum_i dy[i]
        dw = torch.zeros_like(wk)
        for k in range(taps):
            has = torch.as_tensor(table[k] >= 0)
            if has.any():
                dw[k] = f[torch.as_tensor(table[k].astype(np.int64))[has]].T @ dy[has]
        db = dy.sum(0) if has_bias else None
        if fault == "wgrad_counts_dead_rows":                # PAD stale rows behind the count: their table entries and dy are read
            stale = torch.full((PAD, dy.shape[1]), 0.5, dtype=dy.dtype)
            src = f[torch.arange(PAD) % f.shape[0]]
            dw = dw + (src.T @ stale)[None]
            db = None if db is None else db + stale.sum(0)
        if fault == "bias_grad_dropped" and db is not None:
            db = torch.zeros_like(db)
        return dx, dw.reshape(w.shape), db, None, None, None, None


class RuleT:
    """x = (rows (n, C), indices (n, 4), shape): the rulebook's integers are sparse_ref's"""

    def __init__(self, B, dtype=torch.float64, fault=None):
        self.B, self.dtype, self.fault, self.cache, self.record = B, dtype, fault, {}, {}

    def start(self, feats, idx, shape):
        ok = torch.as_tensor(S.keys_of(idx, self.B, shape) >= 0)[:, None]
        return torch.where(ok, feats, torch.zeros((), dtype=self.dtype)), np.asarray(idx, np.int32), tuple(shape)

    def conv(self, x, w, b, kernel, stride, padding, subm, key):
        f, idx, shape = x
        if subm:
            if key not in self.cache:
                self.cache[key] = S.table(idx, idx, self.B, shape, shape, (3, 3, 3), (1, 1, 1), (1, 1, 1))
            t, inv, oidx, osh = self.cache[key], None, idx, shape
        else:
            oidx, osh = S.downsample(idx, self.B, shape, kernel, stride, padding)
            t = S.table(oidx, idx, self.B, shape, osh, kernel, stride, padding)
            inv = inverse_table(idx, oidx, self.B, shape, osh, kernel, stride, padding)
        self.record[key] = dict(indices=oidx, shape=osh, table=t, inverse=inv)
        y = _RuleConv.apply(f, w, b, t, inv, subm, self.fault)
        ok = torch.as_tensor(S.keys_of(oidx, self.B, osh) >= 0)[:, None]
        return torch.where(ok, y, torch.zeros((), dtype=self.dtype)), oidx, osh

    def bn(self, x, g, beta, mean, var, train):
        y, idx, shape = x
        if not train:
            return ((y - mean) / torch.sqrt(var + EPS) * g + beta, idx, shape), None
        n = y.shape[0]
        cnt = float(n + PAD if self.fault == "bn_over_capacity" else n)      # the fault: PAD zero rows join the statistics
        mu = y.sum(0) / cnt
        d = y - mu
        v = ((d * d).sum(0) + (cnt - n) * mu * mu) / cnt
        out = d / torch.sqrt(v + EPS) * g + beta
        unbiased = v if self.fault == "running_var_biased" else v * cnt / (cnt - 1)
        return (out, idx, shape), (mu.detach(), unbiased.detach())

    def act(self, x, residual=None):
        y, idx, shape = x
        return torch.relu(y if residual is None else y + residual[0]), idx, shape

    def dense(self, x):
        f, idx, (D, H, W) = x
        ok = S.keys_of(idx, self.B, (D, H, W)) >= 0
        i = torch.as_tensor(np.asarray(idx, np.int64)[ok])
        out = torch.zeros((self.B, D, H, W, f.shape[1]), dtype=self.dtype).index_put((i[:, 0], i[:, 1], i[:, 2], i[:, 3]), f[torch.as_tensor(ok)])
        return out.permute(0, 4, 1, 2, 3)


def _leaf(v, dtype, grad=True):
    return None if v is None else torch.tensor(np.asarray(v), dtype=dtype, requires_grad=grad)


@torch.enable_grad()                            # whatever the caller (or a test before it) left switched
def layer_train(be, feats, idx, shape, w, b, kernel, stride, padding, subm, cot, input_grad=True):
    """one convolution (bias, no BatchNorm, no ReLU) and its gradients under the dense cotangent `cot` (B, c_out, D', H', W')
    -> {"y": dense output, "dx": (n, c_in) or None, "dW": (taps * c_in, c_out), "db": (c_out) or None} as NumPy arrays"""
    f, wt, bt = _leaf(feats, be.dtype, input_grad), _leaf(w, be.dtype), _leaf(b, be.dtype)
    y = be.dense(be.conv(be.start(f, idx, shape), wt, bt, kernel, stride, padding, subm, "layer"))
    (y * torch.as_tensor(np.asarray(cot)).to(be.dtype)).sum().backward()
    return {"y": y.detach().numpy(), "dx": f.grad.numpy() if input_grad else None, "dW": wt.grad.numpy().reshape(-1, wt.shape[4]),
            "db": None if bt is None else bt.grad.numpy()}


@torch.enable_grad()                            # whatever the caller (or a test before it) left switched
def backbone_train(be, sd, feats, idx, shape, cot=None, train=True):
    """SpMiddleResNetFHD.train_forward from a reference-keyed state_dict -> (outputs {"bev", "conv1" .. "conv4"} dense,
    gradients {key: array} of every parameter under the cotangent `cot` on the BEV map, stats {key: the updated
    running_mean / running_var}). train=False: the BatchNorms in eval mode (no stats)."""
    p = {k: _leaf(v, be.dtype, not k.endswith(("running_mean", "running_var"))) for k, v in sd.items() if not k.endswith("tracked")}
    stats, out, res = {}, {}, 0

    def norm(x, pre):
        y, new = be.bn(x, p[pre + "weight"], p[pre + "bias"], p[pre + "running_mean"], p[pre + "running_var"], train)
        if new is not None:
            for k, v in zip(("running_mean", "running_var"), new):
                stats[pre + k] = ((1 - MOMENTUM) * p[pre + k] + MOMENTUM * v).numpy()
        return y

    x = be.start(torch.as_tensor(np.asarray(feats)).to(be.dtype), idx, shape)
    for name, c, kernel, stride, padding in S.STEMS:
        subm = name == "conv_input"
        x = be.act(norm(be.conv(x, p[f"{name}.0.weight"], None, kernel, stride, padding, subm, "res0" if subm else name), f"{name}.1."))
        if name == "extra_conv":
            break
        seq, key = ("conv1" if subm else name), f"res{res}"
        for j in ((0, 1) if subm else (3, 4)):
            q = f"{seq}.{j}."
            h = be.act(norm(be.conv(x, p[q + "conv1.weight"], p[q + "conv1.bias"], None, None, None, True, key), q + "bn1."))
            x = be.act(norm(be.conv(h, p[q + "conv2.weight"], p[q + "conv2.bias"], None, None, None, True, key), q + "bn2."), x)
        out[seq] = be.dense(x).detach().numpy()
        res += 1
    d = be.dense(x)
    B, C, D, H, W = d.shape
    bev = d.reshape(B, C * D, H, W)
    out["bev"] = bev.detach().numpy()
    grads = {}
    if cot is not None:
        (bev * torch.as_tensor(np.asarray(cot)).to(be.dtype)).sum().backward()
        grads = {k: v.grad.numpy() for k, v in p.items() if v.requires_grad}
    return out, grads, stats


def block_weights(c, tag="trblock"):
    """a reference-keyed state_dict of SparseBasicBlock(c, c)"""
    sd = {}
    for k in (1, 2):
        w, b, bn = S.layer_weights(f"{tag}/{c}/{k}", (3, 3, 3), c, c, True, True)
        sd[f"conv{k}.weight"], sd[f"conv{k}.bias"] = w, b
        for name, v in zip(("weight", "bias", "running_mean", "running_var"), bn):
            sd[f"bn{k}.{name}"] = v
    return sd


@torch.enable_grad()                            # whatever the caller (or a test before it) left switched
def block_train(be, sd, feats, idx, shape, cot):
    """SparseBasicBlock.train_forward in train mode -> (dense output, gradients {key, "x": (n, c)}, updated running stats)"""
    p = {k: _leaf(v, be.dtype, not k.endswith(("running_mean", "running_var"))) for k, v in sd.items()}
    f = _leaf(feats, be.dtype)
    stats = {}

    def norm(x, pre):
        y, new = be.bn(x, p[pre + "weight"], p[pre + "bias"], p[pre + "running_mean"], p[pre + "running_var"], True)
        for k, v in zip(("running_mean", "running_var"), new):
            stats[pre + k] = ((1 - MOMENTUM) * p[pre + k] + MOMENTUM * v).numpy()
        return y

    x = be.start(f, idx, shape)
    h = be.act(norm(be.conv(x, p["conv1.weight"], p["conv1.bias"], None, None, None, True, "b"), "bn1."))
    y = be.dense(be.act(norm(be.conv(h, p["conv2.weight"], p["conv2.bias"], None, None, None, True, "b"), "bn2."), x))
    (y * torch.as_tensor(np.asarray(cot)).to(be.dtype)).sum().backward()
    grads = {k: v.grad.numpy() for k, v in p.items() if v.requires_grad}
    grads["x"] = f.grad.numpy()
    return y.detach().numpy(), grads, stats


def zero_by_batchnorm(key):
    """a convolution's bias in front of a train-mode BatchNorm: its gradient is zero in exact arithmetic (the batch mean
    takes the bias out again), what is computed is rounding noise, and no relative measure applies to it"""
    return key.endswith(("conv1.bias", "conv2.bias"))


def as_rows(a):
    """how a parameter, its gradient or a statistic is judged: a weight as (taps * c_in, c_out) rows; a vector (a bias,
    a BatchNorm parameter, a running statistic) as ONE channel of C rows: a single element is no scale for itself (it can
    cancel to nearly zero, and two equally good fp32 evaluations then differ by any factor relative to it), the vector's
    largest element is"""
    a = np.asarray(a)
    return a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a[:, None]
