"""Float64 restatements of the detector's dense stage (3dal_pytorch_amd/rpn.py; dal3_conv2d_pack / dal3_conv2d of
include/dal3.h): the three layer forms, the BatchNorm fold, the RPN neck and the CenterHead, with the seeded weights and
canvases of tests/golden/rpn.npz (written by tests/golden/gen_rpn.py from the reference's own RPN and CenterHead).

`layer` is a form evaluated in float64 from the UNFOLDED parameters (convolution, then the BatchNorm's own arithmetic):
that it equals the reference modules' .double() outputs is what tests/test_rpn_cpu.py pins. `fold` is the packing's
arithmetic bit for bit (float64 operations in the header's order, one rounding to float32): the impulse tests of
tests/test_gpu_rpn.py derive their expected bits from it. `fault=` plants one wrong reading of the definition at a time.
The measures are pillars_ref.judge's, on (rows, channels) arrays: `rows_of` turns an NCHW map into one."""
import numpy as np

import fold_ref
import pillars_ref as P

synth = P.synth
SEED = 20240917
NECK_EPS, HEAD_EPS = 1e-3, 1e-5
NECK = dict(layer_nums=[3, 5, 5], ds_layer_strides=[1, 2, 2], ds_num_filters=[64, 128, 256], us_layer_strides=[1, 2, 4],
            us_num_filters=[128, 128, 128], num_input_features=64)
TASKS = [dict(num_class=3, class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"])]
COMMON_HEADS = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2)}
HEAD = dict(in_channels=128 * 3, tasks=TASKS, dataset="waymo", weight=2, code_weights=[1.0] * 8, common_heads=COMMON_HEADS)
HEAD_ORDER = ("reg", "height", "dim", "rot", "hm")          # common_heads, then hm: the order SepHead builds them in
CANVASES = {"a": (2, 64, 8, 12), "b": (1, 64, 12, 20)}
OCCUPIED = 0.3
DEAD_CHANNEL = 5                                # of each deblock: channels 5, 133 and 261 of the neck's output
FAULTS = ("neck_eps_1e-5", "taps_flipped", "stride2_shifted", "deconv_transposed", "ups_reordered", "final_bias_dropped",
          "head_eps_1e-3")
MEASURES = P.MEASURES
FLOOR = P.FLOOR

# The GPU tests' bars: multiples of the yardstick (the torch-CPU fp32 layer's or module's own error against the float64
# truth on the same input), by the rule written beside pillars_ref.BARS: the worst ratio of the first MI355X run
# (profiles/rpn_measured.json, DAL3_RPN_RECORD over tests/test_gpu_rpn.py and tests/test_gpu_detector.py in one session)
# x at most 2, rounded up to one significant digit, and under a tenth of the smallest planted-fault ratio of
# tests/test_rpn_cpu.py (3.5e2); a bar comes down or stays, it does not go up. That run (65 rows: 56 single layers, the
# neck, the head and the head alone on three canvases) recorded at worst tensor 1.55 and chan_max 1.55 (both
# layer/64-1/3x32/13x37, one output channel) and chan_rms 1.20 (layer/384-64/3x32/13x37): x 1.94 gives 3, x 2 gives
# 2.4 -> 3. The whole neck and head stayed between 0.75 and 1.32.
BARS = {"tensor": 3.0, "chan_rms": 3.0, "chan_max": 3.0}


def rows_of(y):
    """(B, C, H, W) -> (B * H * W, C): the (rows, channels) layout judge takes"""
    y = np.asarray(y)
    return np.ascontiguousarray(np.moveaxis(y, 1, -1).reshape(-1, y.shape[1]))


def judge(got, truth):
    return P.judge(rows_of(got), rows_of(truth))


def ratios(got, f32, truth):
    return P.ratios(rows_of(got), rows_of(f32), rows_of(truth))


def canvas(tag, shape, occupied=OCCUPIED):
    """a BEV canvas as the reader leaves it: about `occupied` of the cells hold post-ReLU features, the rest +0"""
    B, C, H, W = shape
    live = synth.uniform(SEED, f"canvas/{tag}/live", (B, 1, H, W)) < occupied
    return (synth.uniform(SEED, f"canvas/{tag}/x", shape, 0.0, 2.0) * live).astype(np.float32)


# ------------------------------------------------------------------------------------- weights
def _bn(sd, p, tag, c):
    sd[p + "weight"] = synth.uniform(SEED, tag + "/g", (c,), 0.5, 1.5).astype(np.float32)
    sd[p + "bias"] = synth.uniform(SEED, tag + "/b", (c,), 0.1, 0.5).astype(np.float32)
    sd[p + "running_mean"] = synth.uniform(SEED, tag + "/m", (c,), -0.3, 0.3).astype(np.float32)
    sd[p + "running_var"] = synth.uniform(SEED, tag + "/v", (c,), 0.5, 2.0).astype(np.float32)
    sd[p + "num_batches_tracked"] = np.asarray(7, np.int64)


def _w(tag, shape, fan_in, deconv=False):
    """uniform on [-a, a] with variance 2 / fan_in, which keeps a ReLU chain's rms, minus its mean over the fan-in: the
    inputs are post-ReLU (all positive), and without this a channel's response is mostly sum(w) * mean(x), which leaves
    channels dead or nearly so: a nearly dead channel's own scale is tiny and its relative error says nothing"""
    a = np.sqrt(6.0 / fan_in)
    w = synth.uniform(SEED, tag + "/w", shape, -a, a)
    return (w - w.mean(axis=0 if deconv else tuple(range(1, len(shape))), keepdims=True)).astype(np.float32)


def neck_weights(tag="neck"):
    """a reference-keyed state_dict of the production RPN: seeded uniform weights scaled by fan-in, BatchNorm statistics
    away from (0, 1)"""
    sd, cin = {}, NECK["num_input_features"]
    for i, (n, c) in enumerate(zip(NECK["layer_nums"], NECK["ds_num_filters"])):
        for j in range(n + 1):
            sd[f"blocks.{i}.{3 * j + 1}.weight"] = _w(f"{tag}/b{i}/{j}", (c, cin if j == 0 else c, 3, 3), 9 * (cin if j == 0 else c))
            _bn(sd, f"blocks.{i}.{3 * j + 2}.", f"{tag}/b{i}/{j}", c)
        s, up = NECK["us_layer_strides"][i], NECK["us_num_filters"][i]
        sd[f"deblocks.{i}.0.weight"] = _w(f"{tag}/d{i}", (up, c, 1, 1) if s == 1 else (c, up, s, s), c, deconv=s != 1)
        _bn(sd, f"deblocks.{i}.1.", f"{tag}/d{i}", up)
        cin = c
    # one channel of every upsampled map is dead (a BatchNorm offset far below any response): relu leaves exactly +0
    for i in range(3):
        sd[f"deblocks.{i}.1.bias"][DEAD_CHANNEL] = -60.0
    return sd


def head_weights(tag="head"):
    """a reference-keyed state_dict of the production CenterHead (every convolution has a bias)"""
    sd = {}
    sd["shared_conv.0.weight"] = _w(f"{tag}/s", (64, 384, 3, 3), 9 * 384)
    sd["shared_conv.0.bias"] = synth.uniform(SEED, f"{tag}/s/bias", (64,), -0.2, 0.2).astype(np.float32)
    _bn(sd, "shared_conv.1.", f"{tag}/s", 64)
    for t in range(len(TASKS)):
        heads = dict(COMMON_HEADS, hm=(TASKS[t]["num_class"], 2))
        for name in HEAD_ORDER:
            p, c = f"tasks.{t}.{name}.", heads[name][0]
            sd[p + "0.weight"] = _w(f"{tag}/{t}/{name}/0", (64, 64, 3, 3), 9 * 64)
            sd[p + "0.bias"] = synth.uniform(SEED, f"{tag}/{t}/{name}/0/bias", (64,), -0.2, 0.2).astype(np.float32)
            _bn(sd, p + "1.", f"{tag}/{t}/{name}/1", 64)
            sd[p + "3.weight"] = _w(f"{tag}/{t}/{name}/3", (c, 64, 3, 3), 9 * 64)
            sd[p + "3.bias"] = synth.uniform(SEED, f"{tag}/{t}/{name}/3/bias", (c,), -0.5, 0.5).astype(np.float32)
    return sd


def bn_of(sd, p):
    """the BatchNorm entries under prefix p -> (g, beta, mean, var), or None"""
    return tuple(sd[p + k] for k in ("weight", "bias", "running_mean", "running_var")) if p + "running_var" in sd else None


# ------------------------------------------------------------------------------------- the fold, bit for bit
def fold(w, bias, bn, eps, deconv=False):
    """fold_ref.fold with a Conv2d's (c_out, c_in, k, k) or a ConvTranspose2d's (c_in, c_out, s, s) weight"""
    return fold_ref.fold(w, bias, bn, eps, 1 if deconv else 0)


# ------------------------------------------------------------------------------------- the three forms, float64
def conv3x3(x, w, stride=1, fault=None):
    """sum W[co,ci,ky,kx] * x[b,ci,oy*s+ky-1,ox*s+kx-1], zeros outside -> (B, c_out, (H-1)//s+1, (W-1)//s+1)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, C, H, W = x.shape
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if fault == "taps_flipped":
        w = w[:, :, ::-1, ::-1]
    off = 1 if (fault == "stride2_shifted" and stride == 2) else 0
    xp = np.zeros((B, C, H + 3, W + 3))
    xp[:, :, 1:H + 1, 1:W + 1] = x
    y = np.zeros((B, w.shape[0], OH, OW))
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, ky + off:ky + off + (OH - 1) * stride + 1:stride, kx + off:kx + off + (OW - 1) * stride + 1:stride]
            y += np.einsum("oc,bchw->bohw", w[:, :, ky, kx], win, optimize=True)
    return y


def conv1x1(x, w):
    w = np.asarray(w, np.float64)
    return np.einsum("oc,bchw->bohw", w.reshape(w.shape[0], w.shape[1]), np.asarray(x, np.float64), optimize=True)


def deconv(x, w, s, fault=None):
    """y[b,co,iy*s+dy,ix*s+dx] = sum W[ci,co,dy,dx] * x[b,ci,iy,ix]"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    if fault == "deconv_transposed":
        w = w.transpose(0, 1, 3, 2)
    B, C, H, W = x.shape
    y = np.einsum("codx,bchw->bohdwx", w, x, optimize=True)         # (B, co, H, dy, W, dx)
    return y.reshape(B, w.shape[1], H * s, W * s)


def form(x, w, kind, stride, fault=None):
    """kind: '3x3' | '1x1' | 'deconv'"""
    if kind == "3x3":
        return conv3x3(x, w, stride, fault)
    return conv1x1(x, w) if kind == "1x1" else deconv(x, w, stride, fault)


def layer(x, w, bias, bn, eps, kind, stride, relu, fault=None):
    """Conv + optional eval-mode BatchNorm + optional ReLU in float64, from the unfolded parameters"""
    y = form(x, w, kind, stride, fault)
    if bias is not None:
        y = y + np.asarray(bias, np.float64).reshape(1, -1, 1, 1)
    if bn is not None:
        g, beta, mean, var = (np.asarray(v, np.float64).reshape(1, -1, 1, 1) for v in bn)
        y = (y - mean) / np.sqrt(var + eps) * g + beta
    return np.maximum(y, 0.0) if relu else y


def folded_layer(x, wf, bf, kind, stride, relu):
    """the same layer from FOLDED float32 parameters, in float64: the truth a single launch is judged against"""
    y = form(x, wf, kind, stride) + np.asarray(bf, np.float64).reshape(1, -1, 1, 1)
    return np.maximum(y, 0.0) if relu else y


def _rms_ok(y, what):
    rms = float(np.sqrt((y ** 2).mean()))
    assert 0.1 <= rms <= 10.0, f"{what}: output rms {rms:.3g} left [0.1, 10]: the seeded weights no longer keep the scale"


def neck_f64(sd, x, fault=None):
    """RPN.forward (eval mode, the production configuration) in float64 -> (B, 384, H, W)"""
    eps = 1e-5 if fault == "neck_eps_1e-5" else NECK_EPS
    x, ups = np.asarray(x, np.float64), []
    for i, n in enumerate(NECK["layer_nums"]):
        for j in range(n + 1):
            x = layer(x, sd[f"blocks.{i}.{3 * j + 1}.weight"], None, bn_of(sd, f"blocks.{i}.{3 * j + 2}."), eps, "3x3",
                      NECK["ds_layer_strides"][i] if j == 0 else 1, True, fault)
            _rms_ok(x, f"blocks.{i}.{3 * j + 1}")
        s = NECK["us_layer_strides"][i]
        ups.append(layer(x, sd[f"deblocks.{i}.0.weight"], None, bn_of(sd, f"deblocks.{i}.1."), eps, "1x1" if s == 1 else "deconv",
                         s, True, fault))
        _rms_ok(ups[-1], f"deblocks.{i}")
    if fault == "ups_reordered":
        ups = [ups[1], ups[0], ups[2]]
    return np.concatenate(ups, 1)


def head_f64(sd, x, fault=None):
    """CenterHead.forward (eval mode) in float64 -> [ {head: (B, c, H, W)} per task ]"""
    eps = 1e-3 if fault == "head_eps_1e-3" else HEAD_EPS
    x = layer(x, sd["shared_conv.0.weight"], sd["shared_conv.0.bias"], bn_of(sd, "shared_conv.1."), eps, "3x3", 1, True, fault)
    _rms_ok(x, "shared_conv")
    out = []
    for t in range(len(TASKS)):
        d = {}
        for name in HEAD_ORDER:
            p = f"tasks.{t}.{name}."
            y = layer(x, sd[p + "0.weight"], sd[p + "0.bias"], bn_of(sd, p + "1."), eps, "3x3", 1, True, fault)
            _rms_ok(y, p + "0")
            d[name] = layer(y, sd[p + "3.weight"], None if fault == "final_bias_dropped" else sd[p + "3.bias"], None, eps, "3x3", 1,
                            False, fault)
            _rms_ok(d[name], p + "3")
        out.append(d)
    return out


def head_cat(preds):
    """the head's maps of every task side by side, in HEAD_ORDER -> (B, 11 per task, H, W)"""
    return np.concatenate([np.asarray(d[name]) for d in preds for name in HEAD_ORDER], 1)


# ------------------------------------------------------------------------------------- the layer table and its FLOP
def layer_table(H, W):
    """every layer of neck + head at an (H, W) canvas: (name, kind, stride, c_in, c_out, H_in, W_in)"""
    rows, cin, h, w = [], NECK["num_input_features"], H, W
    for i, (n, c) in enumerate(zip(NECK["layer_nums"], NECK["ds_num_filters"])):
        for j in range(n + 1):
            s = NECK["ds_layer_strides"][i] if j == 0 else 1
            rows.append((f"blocks.{i}.{3 * j + 1}", "3x3", s, cin if j == 0 else c, c, h, w))
            h, w = (h - 1) // s + 1, (w - 1) // s + 1
        s = NECK["us_layer_strides"][i]
        rows.append((f"deblocks.{i}.0", "1x1" if s == 1 else "deconv", s, c, NECK["us_num_filters"][i], h, w))
        cin = c
    rows.append(("shared_conv.0", "3x3", 1, 384, 64, H, W))
    for t in range(len(TASKS)):
        heads = dict(COMMON_HEADS, hm=(TASKS[t]["num_class"], 2))
        for name in HEAD_ORDER:
            rows.append((f"tasks.{t}.{name}.0", "3x3", 1, 64, 64, H, W))
            rows.append((f"tasks.{t}.{name}.3", "3x3", 1, 64, heads[name][0], H, W))
    return rows


def table_flop(H, W, B=1):
    """2 * MACs of the table: per output pixel c_in * taps per output channel (a deconv: per INPUT pixel, s * s outputs)"""
    total = 0
    for _, kind, s, cin, cout, h, w in layer_table(H, W):
        if kind == "3x3":
            total += 2 * ((h - 1) // s + 1) * ((w - 1) // s + 1) * cout * cin * 9
        elif kind == "1x1":
            total += 2 * h * w * cout * cin
        else:
            total += 2 * h * w * cout * s * s * cin
    return B * total
