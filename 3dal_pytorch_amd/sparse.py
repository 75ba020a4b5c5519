"""The sparse 3-D middle of the VoxelNet detector on the GPU through lib3dal_hip.so (dal3_sp_* of include/dal3.h), under the
reference's names, constructor signatures and state_dict keys: `SparseBasicBlock` and `SpMiddleResNetFHD`
(det3d/models/backbones/scn.py), and what they take from spconv 1.x: `SparseConvTensor`, `SubMConv3d`, `SparseConv3d`.

Weights are spconv 1.x's (kD, kH, kW, c_in, c_out) and the operation is a cross-correlation: output site p sums
in[p * stride - padding + k] @ W[k] over the taps whose input site is active. A submanifold layer (kernel 3) keeps its input's
sites and row order; a SparseConv3d's sites are emitted in ascending (b, z, y, x) order. Site counts stay on the device
(`SparseConvTensor.n`, an int64 (1) tensor the later kernels read): the forward never synchronises, every buffer is
capacity-sized, and a level that would exceed its capacity sets _hip.SP_OVERFLOW in `status` and stays in bounds. float32.
`forward` is the eval-mode route (BatchNorm folded into the packs; a train-mode forward is refused). `train_forward` is
the differentiable one: every convolution is a torch.autograd.Function around dal3_sp_conv whose backward runs the data
gradient on the same kernel (the transposed pack on the inverse table) and the weight gradient through dal3_sp_wgrad;
BatchNorm over the live rows (`batch_norm_rows`), ReLU and the residual are stock torch ops. There is no CPU route.

`sparse_precision` on the layers, the block and the backbone ("fp32", the default, | "fp16" | "bf16") picks the MFMA operand
type of the eval-mode convolutions: with a 16-bit one every layer runs dal3_sp_conv_lp on weights rounded once at pack time;
the first layer rounds the float32 voxel features as it stages them, every later layer gathers the 16-bit rows its
producer stored beside (or instead of) the float32 ones (`SparseConvTensor.features16`). Residuals, the returned levels and
the BEV map stay float32; the bookkeeping is the same either way, and `train_forward` ignores the knob.
"""
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from . import _hip
from .pillars import _device_ints
from .rpn import _TORCH16, _PackedLayers, check_precision


def _triple(v):
    return tuple(int(x) for x in v) if isinstance(v, (tuple, list)) else (int(v),) * 3


def out_shape(shape, kernel, stride, padding):
    """floor((in + 2 pad - k) / s) + 1 per axis"""
    return tuple((int(n) + 2 * p - k) // s + 1 for n, k, s, p in zip(shape, kernel, stride, padding))


def candidates(kernel, stride):
    """output sites one input site can belong to: ceil(k / s) per axis"""
    return int(np.prod([-(-k // s) for k, s in zip(kernel, stride)]))


def safe_capacity(in_capacity, batch_size, shape, kernel, stride, padding):
    """the bound no input exceeds: min(candidates per input x input capacity, B x output cells)"""
    return int(min(candidates(kernel, stride) * in_capacity, batch_size * int(np.prod(out_shape(shape, kernel, stride, padding)))))


def _check_grid(batch_size, shape):
    """the library's own bound (sp_grid_ok of csrc/dal3_api.hip), term for term: what passes here is never refused there"""
    if batch_size < 1 or any(n < 1 for n in shape):
        raise ValueError(f"batch_size {batch_size} and spatial_shape {tuple(shape)} must be positive")
    if batch_size > 65535 or any(n > 65536 for n in shape):
        raise ValueError(f"batch_size {batch_size} must be at most 65535 and every axis of {tuple(shape)} at most 65536 cells")
    cells = int(np.prod([int(n) for n in shape], dtype=np.int64))
    if cells >= (2 ** 31 - 1) // batch_size:    # the library's integer division: one cell stricter than B * cells < 2^31 - 1
        raise ValueError(f"B * D * H * W = {batch_size} * {cells} does not fit the 31-bit (sample, cell) key: split the batch")


class SparseConvTensor:
    """features (capacity, C) float32 and indices (capacity, 4) int32 rows [b, z, y, x] on the GPU, spatial_shape (D, H, W),
    batch_size. n: a device int64 (1) tensor, the rows in use (None: all of them). status: the int32 (1) word the kernels OR
    problems into (_hip.SP_*). `sorted` (keys, rows; rows None = the identity) and `indice_dict` are the bookkeeping the
    layers share. features16: optionally the same rows rounded to torch.float16 or torch.bfloat16, (capacity, C), as a
    16-bit layer stores them for the next one to gather; a layer whose float32 rows nobody reads has `features` None."""

    def __init__(self, features, indices, spatial_shape, batch_size, n=None, status=None, features16=None):
        for t, what in ((features, "features"), (indices, "indices")):
            if not torch.is_tensor(t) and not (t is None and what == "features" and features16 is not None):
                raise TypeError(f"{what} must be a tensor")
        rows = (features if features is not None else features16).shape[0]
        if features is not None and (features.dim() != 2 or features.dtype != torch.float32):
            raise ValueError(f"features must be float32 (n, C), got {features.dtype} {tuple(features.shape)}")
        if indices.shape != (rows, 4) or indices.dtype != torch.int32:
            raise ValueError(f"indices must be int32 ({rows}, 4), got {indices.dtype} {tuple(indices.shape)}")
        if features16 is not None:
            if not torch.is_tensor(features16) or features16.dtype not in (torch.float16, torch.bfloat16) or features16.dim() != 2 or \
                    features16.shape[0] != rows or (features is not None and features16.shape != features.shape):
                raise ValueError("features16 must be a float16 or bfloat16 tensor of the features' shape (capacity, C)")
            _hip.require_gpu(features16, "features16")
            features16 = features16.contiguous()
        if features is not None:
            _hip.require_gpu(features, "features")
        _hip.require_gpu(indices, "indices")
        self.features, self.indices = None if features is None else features.contiguous(), indices.contiguous()
        self.features16 = features16
        self.spatial_shape, self.batch_size = tuple(int(v) for v in spatial_shape), int(batch_size)
        if len(self.spatial_shape) != 3:
            raise ValueError("spatial_shape must be (D, H, W)")
        _check_grid(self.batch_size, self.spatial_shape)
        dev = indices.device
        self.n = _device_ints(n, "n", torch.int64, 1, dev)
        self.status = _device_ints(status, "status", torch.int32, 1, dev)
        if self.status is None:
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sorted, self.indice_dict = None, {}

    @property
    def capacity(self):
        return self.indices.shape[0]

    def like(self, features, features16=None):
        """the same sites with other features (what a submanifold layer returns); features16 is the caller's or none"""
        out = SparseConvTensor(features, self.indices, self.spatial_shape, self.batch_size, self.n, self.status, features16)
        out.sorted, out.indice_dict = self.sorted, self.indice_dict
        return out

    def dense(self):
        """(B, C, D, H, W), inactive cells +0; stock torch ops, no synchronisation (rows that are no site go to a spare cell)"""
        D, H, W = self.spatial_shape
        cells = self.batch_size * D * H * W
        i = self.indices.long()
        ok = (i[:, 0] >= 0) & (i[:, 0] < self.batch_size) & (i[:, 1] >= 0) & (i[:, 1] < D) & (i[:, 2] >= 0) & (i[:, 2] < H) & \
            (i[:, 3] >= 0) & (i[:, 3] < W)
        if self.n is not None:
            ok = ok & (torch.arange(self.capacity, device=i.device) < self.n)
        flat = torch.where(ok, ((i[:, 0] * D + i[:, 1]) * H + i[:, 2]) * W + i[:, 3], torch.full_like(i[:, 0], cells))
        out = torch.zeros((cells + 1, self.features.shape[1]), dtype=torch.float32, device=i.device)
        out.index_copy_(0, flat, self.features)
        return out[:cells].reshape(self.batch_size, D, H, W, -1).permute(0, 4, 1, 2, 3).contiguous()


# ------------------------------------------------------------------------------------- the bookkeeping
def _i3(v):
    return (_hip.C.c_int32 * 3)(*[int(x) for x in v])


def sort_sites(x, max_workgroups=0):
    """x.sorted = (keys, rows) of the tensor's sites by ascending key (dal3_sp_sort); flags bad and duplicate rows"""
    if x.sorted is None:
        cap, dev = x.capacity, x.indices.device
        key = torch.empty(cap, dtype=torch.int32, device=dev)
        pos = torch.empty(cap, dtype=torch.int32, device=dev)
        lib = _hip.lib()
        nbytes = lib.dal3_sp_sort_workspace_bytes(cap)
        ws = _hip.workspace(nbytes, dev)
        a = _hip.SpSortArgs(B=x.batch_size, shape=_i3(x.spatial_shape), capacity=cap, n=_hip.ptr(x.n), indices=_hip.ptr(x.indices),
                            sorted_key=_hip.ptr(key), sorted_pos=_hip.ptr(pos), status=_hip.ptr(x.status),
                            max_workgroups=int(max_workgroups), workspace=_hip.ptr(ws), workspace_bytes=nbytes)
        _hip.check(lib.dal3_sp_sort(a, _hip.stream()))
        x.sorted = (key, pos)
    return x.sorted


def neighbour_table(x, out_indices, out_n, out_capacity, shape_out, kernel, stride, padding, max_workgroups=0, table=None):
    """(taps, out_capacity) int32, tap-major: the input row under each tap of each output site, -1 for none (dal3_sp_table)"""
    key, pos = sort_sites(x, max_workgroups)
    taps = int(np.prod(kernel))
    if table is None:
        table = torch.empty((taps, out_capacity), dtype=torch.int32, device=x.indices.device)
    a = _hip.SpTableArgs(B=x.batch_size, in_shape=_i3(x.spatial_shape), out_shape=_i3(shape_out), kernel=_i3(kernel),
                         stride=_i3(stride), padding=_i3(padding), out_capacity=out_capacity, n_out=_hip.ptr(out_n),
                         out_indices=_hip.ptr(out_indices), in_capacity=x.capacity, n_in=_hip.ptr(x.n), in_key=_hip.ptr(key),
                         in_pos=_hip.ptr(pos), table=_hip.ptr(table), max_workgroups=int(max_workgroups))
    _hip.check(_hip.lib().dal3_sp_table(a, _hip.stream()))
    return table


def subm_table(x, indice_key=None, max_workgroups=0):
    """the 27-tap table of a submanifold kernel-3 layer, shared by every layer with the same indice_key"""
    if indice_key is not None and indice_key in x.indice_dict:
        return x.indice_dict[indice_key]
    t = neighbour_table(x, x.indices, x.n, x.capacity, x.spatial_shape, (3, 3, 3), (1, 1, 1), (1, 1, 1), max_workgroups)
    if indice_key is not None:
        x.indice_dict[indice_key] = t
    return t


def downsample(x, kernel, stride, padding, capacity=None, max_workgroups=0, indices=None, keys=None):
    """the output sites of a SparseConv3d -> (an empty-featured description: indices, keys, n, capacity, shape)
    (dal3_sp_downsample). capacity None: the safe bound. indices / keys: caller's buffers (tests put guard rows around them)."""
    shape = out_shape(x.spatial_shape, kernel, stride, padding)
    if any(n < 1 for n in shape):
        raise ValueError(f"a {tuple(kernel)} kernel with stride {tuple(stride)} and padding {tuple(padding)} leaves no cell of {x.spatial_shape}")
    _check_grid(x.batch_size, shape)
    cand = candidates(kernel, stride)
    cap = safe_capacity(x.capacity, x.batch_size, x.spatial_shape, kernel, stride, padding) if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError("capacity must be >= 0")
    dev = x.indices.device
    if indices is None:
        indices = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    if keys is None:
        keys = torch.empty(cap, dtype=torch.int32, device=dev)
    n_out = torch.empty(1, dtype=torch.int64, device=dev)
    lib = _hip.lib()
    nbytes = lib.dal3_sp_downsample_workspace_bytes(x.capacity, cand)
    ws = _hip.workspace(nbytes, dev)
    a = _hip.SpDownsampleArgs(B=x.batch_size, in_shape=_i3(x.spatial_shape), out_shape=_i3(shape), kernel=_i3(kernel),
                              stride=_i3(stride), padding=_i3(padding), in_capacity=x.capacity, n_in=_hip.ptr(x.n),
                              in_indices=_hip.ptr(x.indices), out_capacity=cap, out_indices=_hip.ptr(indices),
                              out_key=_hip.ptr(keys), n_out=_hip.ptr(n_out), status=_hip.ptr(x.status),
                              max_workgroups=int(max_workgroups), workspace=_hip.ptr(ws), workspace_bytes=nbytes)
    _hip.check(lib.dal3_sp_downsample(a, _hip.stream()))
    return indices, keys, n_out, cap, shape


# ------------------------------------------------------------------------------------- the convolution
def pack_layer(conv, bn, status=None, precision="fp32"):
    """fold and pack one layer -> a float32 device tensor (dal3_sp_conv_pack), or for 'fp16' / 'bf16' the uint8 blob of
    dal3_sp_conv_lp_pack. conv: SubMConv3d / SparseConv3d; bn: nn.BatchNorm1d or None. A folded weight that is not finite
    (in the 16-bit type, for a 16-bit pack) sets SP_BAD_WEIGHT in `status` on the device; nothing synchronises."""
    dtype = check_precision(precision)
    L = _hip.fold_layer_struct(conv, bn)
    if bn is not None and not (isinstance(bn, nn.BatchNorm1d) and bn.affine and bn.track_running_stats):
        raise RuntimeError("the norm layer must be an affine nn.BatchNorm1d with running statistics")
    lib = _hip.lib()
    taps = int(np.prod(conv.kernel_size))
    floats = lib.dal3_sp_conv_pack_floats(taps, conv.in_channels, conv.out_channels)
    if not floats:
        raise ValueError(f"the kernel serves c_in 1 .. 8, 16, 32, 64, 128 and c_out 16, 32, 64, 128, not {conv.in_channels} -> "
                         f"{conv.out_channels}")
    eps = float(bn.eps) if bn is not None else 1e-3
    if precision != "fp32":
        buf = torch.empty(lib.dal3_sp_conv_lp_pack_bytes(taps, conv.in_channels, conv.out_channels), dtype=torch.uint8,
                          device=conv.weight.device)
        _hip.check(lib.dal3_sp_conv_lp_pack(L, taps, eps, dtype, _hip.ptr(buf), _hip.ptr(status), _hip.stream()))
        return buf
    buf = torch.empty(floats, dtype=torch.float32, device=conv.weight.device)
    _hip.check(lib.dal3_sp_conv_pack(L, taps, eps, _hip.ptr(buf), _hip.ptr(status), _hip.stream()))
    return buf


def conv(features, table, n_out, packed, c_in, c_out, status, relu=False, residual=None, center_tap=-1, canvas=None,
         out_indices=None, canvas_shape=None, out=None, max_workgroups=0, precision="fp32", features16=None, out16=False,
         rows=True):
    """one dal3_sp_conv launch: features (in_capacity, c_in), table (taps, out_capacity) -> (out_capacity, c_out) rows, or, with
    `canvas` (B, c_out * D, H, W), the BEV store (the rows are then not kept).
    precision 'fp16' / 'bf16': dal3_sp_conv_lp on a pack of that precision. The input is `features` (float32, rounded as it is
    staged) or `features16` (the producer's 16-bit rows; c_in >= 16), exactly one of them. out16: True (allocate) or a
    (out_capacity, c_out) tensor of the 16-bit type that takes q(y); the call then returns (rows or canvas, y16).
    rows=False keeps no float32 rows (out16 is then the only output)."""
    taps, out_cap = table.shape
    if precision != "fp32":
        return _conv_lp(features, table, n_out, packed, c_in, c_out, status, relu, residual, center_tap, canvas, out_indices,
                        canvas_shape, out, max_workgroups, precision, features16, out16, rows)
    check_precision(precision)
    if features16 is not None or out16 is not False or not rows:
        raise ValueError("features16, out16 and rows=False belong to the 16-bit precisions")
    dev = features.device
    if packed.numel() != _hip.lib().dal3_sp_conv_pack_floats(taps, c_in, c_out) or packed.device != dev:
        raise ValueError(f"the packed weights are not those of a {taps}-tap {c_in} -> {c_out} layer on {dev}")
    if features.shape[1] != c_in or features.dtype != torch.float32 or not features.is_contiguous():
        raise ValueError(f"features must be contiguous float32 (n, {c_in}), got {features.dtype} {tuple(features.shape)}")
    if residual is not None and (residual.shape != (out_cap, c_out) or not residual.is_contiguous() or residual.dtype != torch.float32):
        raise ValueError(f"residual must be contiguous float32 ({out_cap}, {c_out})")
    if canvas is None and out is None:
        out = torch.empty((out_cap, c_out), dtype=torch.float32, device=dev)
    a = _hip.SpConvArgs(taps=taps, c_in=c_in, c_out=c_out, relu=1 if relu else 0, center_tap=center_tap,
                        in_capacity=features.shape[0], x=_hip.ptr(features), out_capacity=out_cap, n_out=_hip.ptr(n_out),
                        table=_hip.ptr(table), packed=_hip.ptr(packed), residual=_hip.ptr(residual), y=_hip.ptr(out),
                        canvas=_hip.ptr(canvas), out_indices=_hip.ptr(out_indices), status=_hip.ptr(status),
                        max_workgroups=int(max_workgroups))
    if canvas is not None:
        a.canvas_B = canvas.shape[0]
        a.canvas_shape[:] = [int(v) for v in canvas_shape]
    _hip.check(_hip.lib().dal3_sp_conv(a, _hip.stream()))
    return canvas if canvas is not None else out


def _conv_lp(features, table, n_out, packed, c_in, c_out, status, relu, residual, center_tap, canvas, out_indices, canvas_shape,
             out, max_workgroups, precision, features16, out16, rows):
    """`conv` on 16-bit MFMA operands"""
    dtype, t16 = check_precision(precision), _TORCH16[precision]
    taps, out_cap = table.shape
    dev, lib = table.device, _hip.lib()
    if packed.dtype != torch.uint8 or packed.numel() != lib.dal3_sp_conv_lp_pack_bytes(taps, c_in, c_out) or packed.device != dev:
        raise ValueError(f"the packed weights are not those of a {taps}-tap {c_in} -> {c_out} layer in {precision} on {dev}")
    if (features is None) == (features16 is None):
        raise ValueError("exactly one of features (float32) and features16 is the layer's input")
    if features is not None and (features.shape[1] != c_in or features.dtype != torch.float32 or not features.is_contiguous()):
        raise ValueError(f"features must be contiguous float32 (n, {c_in}), got {features.dtype} {tuple(features.shape)}")
    if features16 is not None and (features16.dim() != 2 or features16.shape[1] != c_in or features16.dtype != t16 or
                                   not features16.is_contiguous() or c_in < 16):
        raise ValueError(f"features16 must be contiguous {t16} (n, {c_in}) with 16 or more channels, got {features16.dtype} "
                         f"{tuple(features16.shape)}")
    if residual is not None and (residual.shape != (out_cap, c_out) or not residual.is_contiguous() or residual.dtype != torch.float32):
        raise ValueError(f"residual must be contiguous float32 ({out_cap}, {c_out})")
    if canvas is None and out is None and rows:
        out = torch.empty((out_cap, c_out), dtype=torch.float32, device=dev)
    y16 = None
    if out16 is True:
        y16 = torch.empty((out_cap, c_out), dtype=t16, device=dev)
    elif out16 is not False:
        y16 = out16
        if not torch.is_tensor(y16) or y16.shape != (out_cap, c_out) or y16.dtype != t16 or not y16.is_contiguous() or y16.device != dev:
            raise ValueError(f"out16 must be a contiguous {t16} ({out_cap}, {c_out}) tensor on {dev}")
    if canvas is None and out is None and y16 is None:
        raise ValueError("the layer has no output: rows=False needs out16 or a canvas")
    x = features if features is not None else features16
    a = _hip.SpConvLpArgs(taps=taps, c_in=c_in, c_out=c_out, relu=1 if relu else 0, center_tap=center_tap, in_capacity=x.shape[0],
                          x=_hip.ptr(features), out_capacity=out_cap, n_out=_hip.ptr(n_out), table=_hip.ptr(table),
                          packed=_hip.ptr(packed), residual=_hip.ptr(residual), y=_hip.ptr(out), canvas=_hip.ptr(canvas),
                          out_indices=_hip.ptr(out_indices), status=_hip.ptr(status), max_workgroups=int(max_workgroups),
                          dtype=dtype, x16=_hip.ptr(features16), y16=_hip.ptr(y16))
    if canvas is not None:
        a.canvas_B = canvas.shape[0]
        a.canvas_shape[:] = [int(v) for v in canvas_shape]
    _hip.check(lib.dal3_sp_conv_lp(a, _hip.stream()))
    first = canvas if canvas is not None else out
    return first if out16 is False else (first, y16)


# ------------------------------------------------------------------------------------- the backward pass
DGRAD_WIDTHS = (16, 32, 64, 128)                # the kernel's output widths: a data gradient has the layer's c_in channels


def transposed_table(x, out_keys, out_n, out_capacity, shape_out, kernel, stride, padding, max_workgroups=0, table=None):
    """(taps, x.capacity) int32, tap-major: the output row that reads input row j under each tap, -1 for none
    (dal3_sp_table_transposed). out_keys: `downsample`'s ascending keys of the output sites"""
    taps = int(np.prod(kernel))
    if table is None:
        table = torch.empty((taps, x.capacity), dtype=torch.int32, device=x.indices.device)
    a = _hip.SpTableTransposedArgs(B=x.batch_size, in_shape=_i3(x.spatial_shape), out_shape=_i3(shape_out), kernel=_i3(kernel),
                                   stride=_i3(stride), padding=_i3(padding), in_capacity=x.capacity, n_in=_hip.ptr(x.n),
                                   in_indices=_hip.ptr(x.indices), out_capacity=out_capacity, n_out=_hip.ptr(out_n),
                                   out_key=_hip.ptr(out_keys), table=_hip.ptr(table), max_workgroups=int(max_workgroups))
    _hip.check(_hip.lib().dal3_sp_table_transposed(a, _hip.stream()))
    return table


def wgrad(features, table, n_out, dy, kernel_size, bias=True, max_workgroups=0):
    """one dal3_sp_wgrad launch: the layer's input rows (in_capacity, c_in), its forward table (taps, out_capacity) and the
    incoming gradient (out_capacity, c_out) -> (dW (kD, kH, kW, c_in, c_out), db (c_out) or None)"""
    taps, out_cap = table.shape
    dev, c_in, c_out = features.device, features.shape[1], dy.shape[1]
    for t, what, rows in ((features, "features", features.shape[0]), (dy, "dy", out_cap)):
        _hip.require_gpu(t, what)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[0] != rows:
            raise ValueError(f"{what} must be contiguous float32 ({rows}, C), got {t.dtype} {tuple(t.shape)}")
    lib = _hip.lib()
    nbytes = lib.dal3_sp_wgrad_workspace_bytes(taps, c_in, c_out, out_cap)
    if not nbytes and out_cap:
        raise ValueError(f"the kernel serves c_in 1 .. 8, 16, 32, 64, 128 and c_out 16, 32, 64, 128, not {c_in} -> {c_out}")
    ws = _hip.workspace(nbytes, dev)
    dw = torch.empty((*kernel_size, c_in, c_out), dtype=torch.float32, device=dev)
    db = torch.empty(c_out, dtype=torch.float32, device=dev) if bias else None
    a = _hip.SpWgradArgs(taps=taps, c_in=c_in, c_out=c_out, in_capacity=features.shape[0], x=_hip.ptr(features), out_capacity=out_cap,
                         n_out=_hip.ptr(n_out), table=_hip.ptr(table), dy=_hip.ptr(dy), dw=_hip.ptr(dw), db=_hip.ptr(db),
                         max_workgroups=int(max_workgroups), workspace=_hip.ptr(ws), workspace_bytes=nbytes)
    _hip.check(lib.dal3_sp_wgrad(a, _hip.stream()))
    return dw, db


def _pack_raw(weight, bias, kernel_size):
    """the unfolded pack of a (kD, kH, kW, c_in, c_out) weight"""
    return pack_layer(SimpleNamespace(weight=weight, bias=bias, in_channels=weight.shape[3], out_channels=weight.shape[4],
                                      kernel_size=kernel_size), None)


class _SparseConvFunction(torch.autograd.Function):
    """y = dal3_sp_conv(features; weight, bias) on a layer's tables. Rows of y, and of the gradients, at or beyond the device
    counts are +0. The backward: dx through dal3_sp_conv on the inverse table with the transposed pack, (dW, db) through
    dal3_sp_wgrad; either is skipped when nothing asks for it."""

    @staticmethod
    def forward(ctx, features, weight, bias, geom):
        features = features.contiguous()
        c_in, c_out = weight.shape[3], weight.shape[4]
        packed = _pack_raw(weight.detach(), None if bias is None else bias.detach(), geom.kernel_size)
        out = torch.zeros((geom.table.shape[1], c_out), dtype=torch.float32, device=features.device)
        conv(features, geom.table, geom.n_out, packed, c_in, c_out, geom.status, center_tap=geom.center, out=out,
             max_workgroups=geom.max_workgroups)
        ctx.save_for_backward(features, weight)
        ctx.geom, ctx.has_bias = geom, bias is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        features, weight = ctx.saved_tensors
        g = ctx.geom
        dy = dy.contiguous()
        c_in, c_out = weight.shape[3], weight.shape[4]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            w = weight.detach()
            wt = (w.flip(0, 1, 2) if g.subm else w).transpose(3, 4).contiguous()
            dx = torch.zeros_like(features)
            conv(dy, g.inverse, g.n_in, _pack_raw(wt, None, g.kernel_size), c_out, c_in, g.status, center_tap=g.center, out=dx,
                 max_workgroups=g.max_workgroups)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = wgrad(features, g.table, g.n_out, dy, g.kernel_size, ctx.has_bias, g.max_workgroups)
        return dx, dw, db, None


def _mask_rows(n, rows, device):
    """(rows, 1) bool: the rows in use; None without a count"""
    return None if n is None else (torch.arange(rows, device=device) < n)[:, None]


def batch_norm_rows(bn, features, n=None):
    """nn.BatchNorm1d `bn` over the first n rows of features (capacity, C); n: a device int64 (1) tensor or None (every row).
    Stock torch ops, differentiable, nothing synchronises. Rows at or beyond n are replaced by +0 before any arithmetic and
    are +0 in the output, so a NaN there reaches neither a statistic nor a gradient. In train mode the statistics are the
    biased batch ones over the n live rows and the running ones take the layer's momentum (the cumulative average with
    momentum None) with the unbiased variance; num_batches_tracked is incremented. In eval mode (a frozen BatchNorm) the
    running statistics are used. nn.BatchNorm1d raises for one row in train mode; that would need the count on the host.
    Here n <= 1 normalises with the batch statistics as they are (one row becomes the bias, no row gives no output) and
    leaves running_mean and running_var untouched; num_batches_tracked still counts the step."""
    if not (isinstance(bn, nn.BatchNorm1d) and bn.affine and bn.track_running_stats):
        raise RuntimeError("the norm layer must be an affine nn.BatchNorm1d with running statistics")
    rows = features.shape[0]
    mask = _mask_rows(n, rows, features.device)
    x = features if mask is None else torch.where(mask, features, torch.zeros((), dtype=features.dtype, device=features.device))
    if bn.training:
        if n is None:
            cnt = torch.full((), float(rows), dtype=features.dtype, device=features.device)
        else:
            cnt = n.clamp(0, rows).to(features.dtype).reshape(())
        den = cnt.clamp(min=1.0)
        mean = x.sum(0) / den
        d = x - mean
        if mask is not None:
            d = torch.where(mask, d, torch.zeros((), dtype=features.dtype, device=features.device))
        var = (d * d).sum(0) / den
        with torch.no_grad():
            bn.num_batches_tracked += 1
            m = 1.0 / bn.num_batches_tracked.to(features.dtype) if bn.momentum is None else bn.momentum
            m = torch.where(cnt > 1, m * torch.ones_like(cnt), torch.zeros_like(cnt))
            bn.running_mean += m * (mean - bn.running_mean)
            bn.running_var += m * (var * (cnt / (cnt - 1).clamp(min=1.0)) - bn.running_var)
    else:
        mean, var = bn.running_mean, bn.running_var
        d = x - mean
    y = d / torch.sqrt(var + bn.eps) * bn.weight + bn.bias
    return y if mask is None else torch.where(mask, y, torch.zeros((), dtype=y.dtype, device=y.device))


class _SparseLayers(_PackedLayers):
    """_PackedLayers of the sparse middle's modules. `sparse_precision` ('fp32', the default, | 'fp16' | 'bf16') is the MFMA
    operand type of the eval-mode convolutions; it is part of the cache's key, so changing it repacks, and a container sets
    its children. (Not `precision`: that name is the dense stage's knob, which leaves this stage alone.) train_forward
    ignores it."""

    def __init__(self):
        super().__init__()
        self._sparse_precision = "fp32"

    @property
    def sparse_precision(self):
        return self._sparse_precision

    @sparse_precision.setter
    def sparse_precision(self, value):
        check_precision(value)
        for m in self.modules():
            if isinstance(m, _SparseLayers):
                m._sparse_precision = value

    def _pack_key(self):
        return self._sparse_precision

    def _pack(self, plan):
        return [pack_layer(c, bn, precision=self._sparse_precision) for c, bn in plan]


class _SparseConv(_SparseLayers):
    """a parameter container with spconv 1.x's shapes: weight (kD, kH, kW, c_in, c_out), bias (c_out) or None"""
    subm = False

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None, **kwargs):
        super().__init__()
        if _triple(dilation) != (1, 1, 1) or groups != 1:
            raise NotImplementedError("dilation and groups other than 1 are not served")
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size, self.stride, self.padding = _triple(kernel_size), _triple(stride), _triple(padding)
        self.indice_key = indice_key
        self.weight = nn.Parameter(torch.empty(*self.kernel_size, self.in_channels, self.out_channels))
        self.bias = nn.Parameter(torch.empty(self.out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        fan_in = self.in_channels * int(np.prod(self.kernel_size))
        bound = 1.0 / np.sqrt(fan_in)
        nn.init.uniform_(self.weight, -bound * np.sqrt(3.0), bound * np.sqrt(3.0))
        if self.bias is not None:
            nn.init.uniform_(self.bias, -bound, bound)

    def _plan(self):
        return [(self, None)]

    def run(self, x, packed, relu=False, residual=None, capacity=None, max_workgroups=0, canvas=False, rows=True, out16=False):
        """the layer on x with the given pack (its own, or one with a BatchNorm folded in) -> SparseConvTensor, or the
        (B, c_out * D, H, W) BEV map with canvas=True. With a 16-bit `sparse_precision` (which `packed` must be of) the layer
        gathers x.features16 where x has them (and 16 or more channels), x.features otherwise; out16: the output also carries
        features16 = q(features); rows=False: only those."""
        if self.subm:
            if self.kernel_size != (3, 3, 3) or self.stride != (1, 1, 1):
                raise NotImplementedError("SubMConv3d is served with kernel 3 and stride 1")
            table = subm_table(x, self.indice_key, max_workgroups)
            indices, n_out, shape, center = x.indices, x.n, x.spatial_shape, 13
        else:
            indices, keys, n_out, cap, shape = downsample(x, self.kernel_size, self.stride, self.padding, capacity, max_workgroups)
            table = neighbour_table(x, indices, n_out, cap, shape, self.kernel_size, self.stride, self.padding, max_workgroups)
            center = -1
        kw = dict(relu=relu, residual=residual, center_tap=center, max_workgroups=max_workgroups)
        feats, y16 = x.features, None
        if self._sparse_precision != "fp32":
            f16 = x.features16 if self.in_channels >= 16 else None
            if f16 is not None:
                feats = None
            kw.update(precision=self._sparse_precision, features16=f16)
            if not canvas:
                kw.update(out16=bool(out16), rows=rows)
        elif out16 or not rows:
            raise ValueError("out16 and rows=False belong to a 16-bit sparse_precision")
        if canvas:
            D, H, W = shape
            bev = torch.empty((x.batch_size, self.out_channels * D, H, W), dtype=torch.float32, device=x.indices.device)
            return conv(feats, table, n_out, packed, self.in_channels, self.out_channels, x.status, canvas=bev,
                        out_indices=indices, canvas_shape=shape, **kw)
        y = conv(feats, table, n_out, packed, self.in_channels, self.out_channels, x.status, **kw)
        if out16:
            y, y16 = y
        if self.subm:
            return x.like(y, y16)
        out = SparseConvTensor(y, indices, shape, x.batch_size, n_out, x.status, y16)
        out.sorted = (keys, None)               # emitted in key order
        return out

    def forward(self, x, capacity=None, max_workgroups=0):
        _refuse_training(self)
        with torch.no_grad():
            return self.run(x, self.packed()[0], capacity=capacity, max_workgroups=max_workgroups)

    def train_forward(self, x, capacity=None, max_workgroups=0):
        """the differentiable layer: y = conv(x) + bias with gradients to x.features, weight and bias; no BatchNorm, no
        ReLU. A SparseConv3d's inverse table is built with the forward one when the input asks for a gradient."""
        need_dx = torch.is_grad_enabled() and x.features.requires_grad
        if need_dx and self.in_channels not in DGRAD_WIDTHS:
            raise RuntimeError(f"{type(self).__name__} with {self.in_channels} input channels has no data gradient (the kernel "
                               f"produces {DGRAD_WIDTHS} channels): its input features must not require grad")
        _hip.require_gpu(x.features, "features")
        g = SimpleNamespace(subm=self.subm, kernel_size=self.kernel_size, n_in=x.n, status=x.status, max_workgroups=max_workgroups,
                            inverse=None)
        if self.subm:
            if self.kernel_size != (3, 3, 3) or self.stride != (1, 1, 1):
                raise NotImplementedError("SubMConv3d is served with kernel 3 and stride 1")
            g.table = g.inverse = subm_table(x, self.indice_key, max_workgroups)      # the inverse: the same table, taps mirrored
            g.n_out, g.center = x.n, 13
            return x.like(_SparseConvFunction.apply(x.features, self.weight, self.bias, g))
        indices, keys, n_out, cap, shape = downsample(x, self.kernel_size, self.stride, self.padding, capacity, max_workgroups)
        g.table = neighbour_table(x, indices, n_out, cap, shape, self.kernel_size, self.stride, self.padding, max_workgroups)
        if need_dx:
            g.inverse = transposed_table(x, keys, n_out, cap, shape, self.kernel_size, self.stride, self.padding, max_workgroups)
        g.n_out, g.center = n_out, -1
        out = SparseConvTensor(_SparseConvFunction.apply(x.features, self.weight, self.bias, g), indices, shape, x.batch_size, n_out,
                               x.status)
        out.sorted = (keys, None)
        out.rulebook = (g.table, g.inverse)                 # the level's tables, the inverse beside the forward one
        return out


class SubMConv3d(_SparseConv):
    """spconv.SubMConv3d, kernel 3: the output sites are the input sites in the same row order; `padding` plays no part"""
    subm = True


class SparseConv3d(_SparseConv):
    """spconv.SparseConv3d: forward(x, capacity=None) — capacity: rows of the output (None: the safe bound)"""


def _refuse_training(m):
    if m.training:
        raise RuntimeError(f"{type(m).__name__} is the eval-mode forward (call .eval()): training and the backward are not built")


def _norm(cfg, c):
    """det3d/models/utils/norm.py for BN1d"""
    cfg = dict(type="BN1d", eps=1e-3, momentum=0.01) if cfg is None else dict(cfg)
    kind = cfg.pop("type")
    cfg.pop("requires_grad", None)
    if kind not in ("BN1d", "BN"):
        raise KeyError(f"norm layer type {kind!r} (BN1d)")
    return nn.BatchNorm1d(c, eps=cfg.get("eps", 1e-5), momentum=cfg.get("momentum", 0.1))


class SparseBasicBlock(_SparseLayers):
    """scn.py:37-80: relu(bn2(conv2(relu(bn1(conv1(x))))) + x); both convolutions are submanifold and have a bias"""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, norm_cfg=None, downsample=None, indice_key=None):
        super().__init__()
        if downsample is not None or stride != 1 or inplanes != planes:
            raise NotImplementedError("SparseBasicBlock is served with stride 1, equal widths and no downsample")
        self.conv1 = SubMConv3d(inplanes, planes, 3, stride=1, padding=1, bias=True, indice_key=indice_key)
        self.bn1 = _norm(norm_cfg, planes)
        self.relu = nn.ReLU()
        self.conv2 = SubMConv3d(planes, planes, 3, padding=1, bias=True, indice_key=indice_key)
        self.bn2 = _norm(norm_cfg, planes)
        self.downsample, self.stride = downsample, stride

    def _plan(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2)]

    def forward(self, x, max_workgroups=0):
        _refuse_training(self)
        with torch.no_grad():
            p1, p2 = self.packed()
            if self._sparse_precision != "fp32":
                if x.features is None:
                    raise ValueError("the block's residual is its input's float32 rows: the input has none")
                # conv1's rows are read by conv2 alone: 16-bit only; conv2's are the next residual and the next input
                out = self.conv1.run(x, p1, relu=True, max_workgroups=max_workgroups, rows=False, out16=True)
                return self.conv2.run(out, p2, relu=True, residual=x.features, max_workgroups=max_workgroups, out16=True)
            out = self.conv1.run(x, p1, relu=True, max_workgroups=max_workgroups)
            return self.conv2.run(out, p2, relu=True, residual=x.features, max_workgroups=max_workgroups)

    def train_forward(self, x, max_workgroups=0):
        """the same block, differentiable: BatchNorm by its mode over the live rows (batch_norm_rows)"""
        out = self.conv1.train_forward(x, max_workgroups=max_workgroups)
        out = x.like(torch.relu(batch_norm_rows(self.bn1, out.features, x.n)))
        out = self.conv2.train_forward(out, max_workgroups=max_workgroups)
        f = torch.relu(batch_norm_rows(self.bn2, out.features, x.n) + x.features)
        mask = _mask_rows(x.n, x.capacity, f.device)
        return x.like(f if mask is None else torch.where(mask, f, torch.zeros((), dtype=f.dtype, device=f.device)))


class SpMiddleResNetFHD(_SparseLayers):
    """scn.py:83-177. forward(voxel_features, coors, batch_size, input_shape, n_voxels=None) -> (bev (B, 128 * D', H', W'),
    {conv1 .. conv4: SparseConvTensor}). n_voxels: a device int64 (1) tensor (VoxelizeResult.n_pillars), the rows in use;
    without it every row is a voxel. `capacities`: {"conv2" | "conv3" | "conv4" | "extra_conv": rows} for the strided
    levels (default: the safe bound of sparse.safe_capacity). `last_status` is the status word of the last forward."""

    def __init__(self, num_input_features=128, norm_cfg=None, name="SpMiddleResNetFHD", **kwargs):
        super().__init__()
        self.name = name
        self.dcn, self.zero_init_residual = None, False
        self.capacities = kwargs.pop("capacities", None)         # ds_factor and the like are swallowed
        c = int(num_input_features)

        def block(w, key):
            return SparseBasicBlock(w, w, norm_cfg=norm_cfg, indice_key=key)

        self.conv_input = nn.Sequential(SubMConv3d(c, 16, 3, bias=False, indice_key="res0"), _norm(norm_cfg, 16), nn.ReLU(inplace=True))
        self.conv1 = nn.Sequential(block(16, "res0"), block(16, "res0"))
        self.conv2 = nn.Sequential(SparseConv3d(16, 32, 3, 2, padding=1, bias=False), _norm(norm_cfg, 32), nn.ReLU(inplace=True),
                                   block(32, "res1"), block(32, "res1"))
        self.conv3 = nn.Sequential(SparseConv3d(32, 64, 3, 2, padding=1, bias=False), _norm(norm_cfg, 64), nn.ReLU(inplace=True),
                                   block(64, "res2"), block(64, "res2"))
        self.conv4 = nn.Sequential(SparseConv3d(64, 128, 3, 2, padding=[0, 1, 1], bias=False), _norm(norm_cfg, 128),
                                   nn.ReLU(inplace=True), block(128, "res3"), block(128, "res3"))
        self.extra_conv = nn.Sequential(SparseConv3d(128, 128, (3, 1, 1), (2, 1, 1), bias=False), _norm(norm_cfg, 128), nn.ReLU())
        self.last_status = None

    STEMS = ("conv_input", "conv2", "conv3", "conv4", "extra_conv")

    def _plan(self):
        return [(getattr(self, s)[0], getattr(self, s)[1]) for s in self.STEMS]

    def forward(self, voxel_features, coors, batch_size, input_shape, n_voxels=None, capacities=None, max_workgroups=0):
        _refuse_training(self)
        with torch.no_grad():
            sparse_shape = tuple(int(v) for v in (np.array(input_shape[::-1]) + [1, 0, 0]))
            if not torch.is_tensor(coors) or not torch.is_tensor(voxel_features):
                raise TypeError("voxel_features and coors must be tensors")
            x = SparseConvTensor(voxel_features, coors.int(), sparse_shape, batch_size, n=n_voxels)
            self.last_status = x.status
            caps = dict(self.capacities or {}, **(capacities or {}))
            packs = dict(zip(self.STEMS, self.packed()))
            kw = dict(max_workgroups=max_workgroups)
            # on 16-bit operands a stem writes its float32 rows (the next residual) and their 16-bit twin (the next input)
            stem = dict(kw, out16=True) if self._sparse_precision != "fp32" else kw
            x = self.conv_input[0].run(x, packs["conv_input"], relu=True, **stem)
            out = {}
            for name in ("conv1", "conv2", "conv3", "conv4"):
                seq = getattr(self, name)
                blocks = list(seq)
                if name != "conv1":
                    x = seq[0].run(x, packs[name], relu=True, capacity=caps.get(name), **stem)
                    blocks = blocks[3:]
                for b in blocks:
                    x = b(x, **kw)
                out[name] = x
            bev = self.extra_conv[0].run(x, packs["extra_conv"], relu=True, capacity=caps.get("extra_conv"), canvas=True, **kw)
            return bev, out

    def train_forward(self, voxel_features, coors, batch_size, input_shape, n_voxels=None, capacities=None, max_workgroups=0):
        """forward's arguments and outputs, differentiable in every parameter (and in voxel_features when the first layer
        has 16 or more input channels): BatchNorm by its mode over the live rows, the BEV map through .dense(). Nothing
        synchronises, in either direction."""
        sparse_shape = tuple(int(v) for v in (np.array(input_shape[::-1]) + [1, 0, 0]))
        if not torch.is_tensor(coors) or not torch.is_tensor(voxel_features):
            raise TypeError("voxel_features and coors must be tensors")
        x = SparseConvTensor(voxel_features, coors.int(), sparse_shape, batch_size, n=n_voxels)
        self.last_status = x.status
        caps = dict(self.capacities or {}, **(capacities or {}))
        kw = dict(max_workgroups=max_workgroups)

        def stem(name, x):
            seq = getattr(self, name)
            y = seq[0].train_forward(x, **(kw if name == "conv_input" else dict(kw, capacity=caps.get(name))))
            return y.like(torch.relu(batch_norm_rows(seq[1], y.features, y.n)))

        x = stem("conv_input", x)
        out = {}
        for name in ("conv1", "conv2", "conv3", "conv4"):
            blocks = list(getattr(self, name))
            if name != "conv1":
                x = stem(name, x)
                blocks = blocks[3:]
            for b in blocks:
                x = b.train_forward(x, **kw)
            out[name] = x
        d = stem("extra_conv", x).dense()
        B, C, D, H, W = d.shape
        return d.reshape(B, C * D, H, W), out
