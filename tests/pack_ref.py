"""The packed-weight blobs of the detector's MFMA layers, built in numpy from FOLDED float32 parameters (fold_ref.fold)
by the layouts the kernels' header comments document, and taken apart again. tests/test_gpu_pack.py compares them word
for word with what the device packers write.

dense (csrc/dal3_conv2d.hip): the folded bias of every GEMM row, n_tiles * 32 floats, then the fragments
[out tile][8 input channels][tap][lane] float4: element e of a lane is row 32 ot + (lane & 31), channel
8 c8 + 2 e + (lane >> 5). A transposed convolution (weight (c_in, c_out, s, s)) is the 1-tap form with c_out * s * s
rows, row = (co * s + dy) * s + dx. Rows and channels beyond the layer's are +0.

sparse (csrc/dal3_spconv.hip): 64 floats of head (word 0 the non-finite flag), the folded bias, mt * 32 floats, then
[tap][k-step group s4][out tile][lane] float4: element e of a lane is channel 32 mt + (lane & 31) of the output and
input (lane >> 5) * CP / 2 + 4 s4 + e of the CP zero-padded inputs (CP = 8 up to 8 inputs). Weight (kD, kH, kW, c_in, c_out).

RoI head (csrc/dal3_roi.hip): the layers' dense 1x1 blobs one after another."""
import numpy as np

SUB = {"3x3": 1, "1x1": 1, "deconv2": 4, "deconv4": 16}
SP_HEAD = 64


def _dense_gemm(wf, kind):
    """-> A (rows, c_in, taps) float32: the GEMM's left operand, row-major by GEMM row"""
    wf = np.asarray(wf, np.float32)
    if SUB[kind] == 1:
        return wf.reshape(wf.shape[0], wf.shape[1], -1)
    return wf.reshape(wf.shape[0], -1).T[:, :, None]             # (c_in, c_out * s * s) -> (rows, c_in, 1)


def _dense_index(rows, c_in, taps):
    n_tiles, nc8 = -(-rows // 32), -(-c_in // 8)
    ot, c8, tap, lane, e = np.meshgrid(np.arange(n_tiles), np.arange(nc8), np.arange(taps), np.arange(64), np.arange(4), indexing="ij")
    return n_tiles, 32 * ot + (lane & 31), 8 * c8 + 2 * e + (lane >> 5), tap


def dense_blob(wf, bf, kind):
    A = _dense_gemm(wf, kind)
    rows, c_in, taps = A.shape
    n_tiles, row, ci, tap = _dense_index(rows, c_in, taps)
    bias = np.zeros(n_tiles * 32, np.float32)
    bias[:rows] = np.repeat(np.asarray(bf, np.float32), SUB[kind])
    pad = np.zeros((n_tiles * 32, row.shape[1] * 8, taps), np.float32)
    pad[:rows, :c_in] = A
    return np.concatenate([bias, pad[row, ci, tap].ravel()])


def dense_unblob(blob, kind, w_shape):
    """-> (W' shaped w_shape, b' (c_out)); asserts that everything outside the layer is +0"""
    sub = SUB[kind]
    c_out, c_in = (w_shape[0], w_shape[1]) if sub == 1 else (w_shape[1], w_shape[0])
    rows, taps = c_out * sub, int(np.prod(w_shape[2:])) if sub == 1 else 1
    n_tiles, row, ci, tap = _dense_index(rows, c_in, taps)
    blob = np.asarray(blob, np.float32)
    assert blob.size == n_tiles * 32 + row.size
    bias, frag = blob[:n_tiles * 32], blob[n_tiles * 32:].reshape(row.shape)
    pad = np.full((n_tiles * 32, row.shape[1] * 8, taps), np.nan, np.float32)
    pad[row, ci, tap] = frag
    assert not np.isnan(pad).any(), "an element of the GEMM operand has no place in the blob"
    outside = pad.copy()
    outside[:rows, :c_in] = 0
    assert not outside.view(np.uint32).any() and not bias[rows:].view(np.uint32).any()
    assert np.array_equal(bias[:rows].reshape(c_out, sub), np.repeat(bias[:rows:sub, None], sub, 1))
    A = pad[:rows, :c_in]
    wf = A.reshape(w_shape) if sub == 1 else A[:, :, 0].T.reshape(w_shape)
    return wf, bias[:rows:sub].copy()


def _sparse_index(taps, c_in, c_out):
    cp, mt = (8 if c_in <= 8 else c_in), -(-c_out // 32)
    tap, s4, m, lane, e = np.meshgrid(np.arange(taps), np.arange(cp // 8), np.arange(mt), np.arange(64), np.arange(4), indexing="ij")
    return cp, mt, tap, (lane >> 5) * (cp // 2) + 4 * s4 + e, 32 * m + (lane & 31)


def sparse_blob(wf, bf):
    wf = np.asarray(wf, np.float32)
    c_in, c_out = wf.shape[-2:]
    w3 = wf.reshape(-1, c_in, c_out)
    cp, mt, tap, ci, co = _sparse_index(w3.shape[0], c_in, c_out)
    bias = np.zeros(mt * 32, np.float32)
    bias[:c_out] = bf
    pad = np.zeros((w3.shape[0], cp, mt * 32), np.float32)
    pad[:, :c_in, :c_out] = w3
    return np.concatenate([np.zeros(SP_HEAD, np.float32), bias, pad[tap, ci, co].ravel()])


def sparse_unblob(blob, w_shape):
    c_in, c_out = w_shape[-2:]
    taps = int(np.prod(w_shape[:-2]))
    cp, mt, tap, ci, co = _sparse_index(taps, c_in, c_out)
    blob = np.asarray(blob, np.float32)
    assert blob.size == SP_HEAD + mt * 32 + tap.size
    bias, frag = blob[SP_HEAD:SP_HEAD + mt * 32], blob[SP_HEAD + mt * 32:].reshape(tap.shape)
    pad = np.full((taps, cp, mt * 32), np.nan, np.float32)
    pad[tap, ci, co] = frag
    assert not np.isnan(pad).any(), "an element of the GEMM operand has no place in the blob"
    outside = pad.copy()
    outside[:, :c_in, :c_out] = 0
    assert not outside.view(np.uint32).any() and not bias[c_out:].view(np.uint32).any()
    return pad[:, :c_in, :c_out].reshape(w_shape), bias[:c_out].copy()


def roi_blob(layers):
    """layers: [(W' (c_out, c_in), b' (c_out))] in dal3_roi_pack's order"""
    return np.concatenate([dense_blob(np.asarray(wf)[:, :, None, None], bf, "1x1") for wf, bf in layers])


# ------------------------------------------------------------------------------------- the seeded cases
SEED = 20241101
# (name, weight shape, output-channel axis, bias, BatchNorm). The smallest shapes that reach every branch of the packers:
# ragged input channels (5, 9, 3 of 8), a ragged second out tile (33), one and two tiles, 40 and 48 deconv rows
DENSE = (("3x3", (33, 5, 3, 3), 0, True, True), ("3x3", (32, 16, 3, 3), 0, True, False), ("1x1", (8, 9, 1, 1), 0, False, True),
         ("deconv2", (9, 10, 2, 2), 1, False, True), ("deconv4", (3, 3, 4, 4), 1, True, False))
# 1 .. 8 inputs (the padded first layer), 16 -> 32, and the widest layer with 3 taps
SPARSE = (((3, 3, 3, 5, 16), False, True), ((3, 3, 3, 16, 32), True, False), ((3, 1, 1, 128, 128), True, True))
# (c_in, SHARED_FC, CLS_FC, REG_FC, code_size): BatchNorm layers without a bias, final layers with a bias and no BatchNorm
ROI = ((20, (48, 16), (16,), (32,), 7), (9, (16,), (16,), (16,), 9))


def layer_params(tag, w_shape, channel_axis, bias, bn):
    """-> (w, bias or None, (g, beta, mean, var) or None, eps), float32, seeded by the tag; var in [0.5, 2]"""
    rng = np.random.default_rng([SEED] + [ord(c) for c in tag])
    c_out = w_shape[channel_axis]
    u = lambda lo, hi: rng.uniform(lo, hi, c_out).astype(np.float32)
    w = rng.standard_normal(w_shape).astype(np.float32)
    b = u(-0.5, 0.5) if bias else None
    stats = (u(0.5, 1.5) * rng.choice(np.float32([-1, 1]), c_out), u(-0.5, 0.5), u(-0.5, 0.5), u(0.5, 2.0)) if bn else None
    return w, b, stats, float(rng.uniform(1e-5, 1e-3))


def roi_params(case):
    """the layers of a RoI head in dal3_roi_pack's order (shared, cls with its final layer, reg with its final layer)
    -> [layer_params(...)] with (c_out, c_in, 1) weights"""
    c_in, shared, cls, reg, code = ROI[case]
    out, pre = [], c_in
    for k, w in enumerate(shared):
        out.append(layer_params(f"roi{case}/shared{k}", (w, pre, 1), 0, False, True))
        pre = w
    for name, widths, last in (("cls", cls, 1), ("reg", reg, code)):
        p = pre
        for k, w in enumerate(widths):
            out.append(layer_params(f"roi{case}/{name}{k}", (w, p, 1), 0, False, True))
            p = w
        out.append(layer_params(f"roi{case}/{name}_out", (last, p, 1), 0, True, False))
    return out
