"""The detector's dense stage on the GPU through lib3dal_hip.so (dal3_conv2d_pack / dal3_conv2d, include/dal3.h), under
the reference's names, constructor signatures and state_dict keys: `RPN` (det3d/models/necks/rpn.py), `SepHead` and
`CenterHead` (det3d/models/bbox_heads/center_head.py:65-110, 167-244).

The modules hold the reference's own children (nn.Conv2d, nn.BatchNorm2d, nn.ConvTranspose2d at the reference's positions
in their Sequentials), so a checkpoint loads strictly. In eval mode every layer the kernel serves — Conv 3x3 of stride 1
or 2 with one ring of zero padding, Conv 1x1, ConvTranspose k = s in {2, 4}, each with an optional eval-mode BatchNorm2d
and ReLU — runs dal3_conv2d on weights folded and packed once (a cache invalidated by load_state_dict / train / _apply
and the tensors' version stamps); the three upsampled maps are written into channel slices of one tensor, and so are the
head's maps (they are views, not NCHW-contiguous tensors). `composite()` is the same definition in stock torch ops: it
runs in train mode and for whatever the kernel does not serve (a strided-convolution deblock, GroupNorm, other kernel
sizes). There is no quiet fallback on the GPU route: a module that `hip_serves()` raises if its inputs are not on the GPU.

`precision` on `RPN` and `CenterHead` ("fp32", the default, | "fp16" | "bf16") picks the MFMA operand type of that kernel
route: with a 16-bit one every layer runs dal3_conv2d_lp on weights rounded once at pack time and activations rounded as
they are staged, accumulating in fp32; the maps stay float32 either way.

`RPN.train_forward` / `CenterHead.train_forward` are `composite()`'s graph with every convolution on the HIP kernels, forward
and backward (`_Conv2dFunction`: dal3_conv2d on the raw pack, dal3_conv2d_dgrad, dal3_conv2d_wgrad), float32, BatchNorm /
ReLU / torch.cat stock: the opt-in training route (`dense="hip"` of detector.VoxelNet.first_stage_loss). `forward()` in train
mode stays the composite.
"""
import copy

import numpy as np
import torch
from torch import nn

from . import _heads, _hip

KIND_TAPS = {_hip.CONV2D_3X3: 9, _hip.CONV2D_1X1: 1, _hip.CONV2D_DECONV2: 1, _hip.CONV2D_DECONV4: 1}
KIND_SUB = {_hip.CONV2D_3X3: 1, _hip.CONV2D_1X1: 1, _hip.CONV2D_DECONV2: 4, _hip.CONV2D_DECONV4: 16}


def build_norm_layer(cfg, num_features):
    """det3d/models/utils/norm.py for the types the neck is configured with: BN -> nn.BatchNorm2d, GN -> nn.GroupNorm"""
    cfg = dict(cfg)
    kind = cfg.pop("type")
    cfg.pop("requires_grad", None)
    if kind == "BN":
        return nn.BatchNorm2d(num_features, eps=cfg.get("eps", 1e-5), momentum=cfg.get("momentum", 0.1))
    if kind == "GN":
        return nn.GroupNorm(cfg["num_groups"], num_features, eps=cfg.get("eps", 1e-5))
    raise KeyError(f"norm layer type {kind!r} (BN or GN)")


def layer_kind(conv):
    """(kind, stride) of the dal3_conv2d form that serves this module, or None"""
    if isinstance(conv, nn.ConvTranspose2d):
        k, s = conv.kernel_size, conv.stride
        ok = (k[0] == k[1] == s[0] == s[1] and k[0] in (2, 4) and conv.padding == (0, 0) and conv.output_padding == (0, 0)
              and conv.dilation == (1, 1) and conv.groups == 1)
        return ({2: _hip.CONV2D_DECONV2, 4: _hip.CONV2D_DECONV4}[k[0]], k[0]) if ok else None
    if not isinstance(conv, nn.Conv2d) or conv.groups != 1 or conv.dilation != (1, 1) or conv.padding_mode != "zeros":
        return None
    k, s = conv.kernel_size, conv.stride
    if k == (1, 1) and s == (1, 1) and conv.padding == (0, 0):
        return _hip.CONV2D_1X1, 1
    if k == (3, 3) and s[0] == s[1] and s[0] in (1, 2):
        return _hip.CONV2D_3X3, s[0]             # the caller vouches for the one ring of zeros (padding=1 or a ZeroPad2d(1))
    return None


def _norm_ok(bn):
    return bn is None or (isinstance(bn, nn.BatchNorm2d) and bn.affine and bn.track_running_stats)


PRECISIONS = ("fp32", "fp16", "bf16")
_TORCH16 = {"fp16": torch.float16, "bf16": torch.bfloat16}


def check_precision(precision):
    """'fp32' | 'fp16' | 'bf16' -> the DAL3_* dtype (_heads.dtype_of's names and mapping); 'f16x3' belongs to the point
    heads and is refused here"""
    dtype = _heads.dtype_of(precision)
    if precision not in PRECISIONS:
        raise ValueError(f"precision {precision!r}: the detector's dense stage runs on 'fp32', 'fp16' or 'bf16' MFMA operands "
                         "('f16x3' is an arithmetic of the point heads only)")
    return dtype


def _lp_fragments(buf, kind, c_out, precision):
    """the fragment part of a dal3_conv2d_lp_pack blob (behind the float32 biases of its whole 32-row tiles) as the 16-bit type"""
    n_tiles = -(-c_out * KIND_SUB[kind] // 32)
    return buf[n_tiles * 32 * 4:].view(_TORCH16[precision])


def refuse_nonfinite_weights(packs, layers, precision):
    """packs: dal3_conv2d_lp_pack blobs; layers: their (kind, c_out, name). A folded weight that is not finite in the 16-bit
    type is refused here, on the PACKED values (so exactly what the kernel would read), with one device->host sync for all
    the blobs of a packing, as _hip.check_f16x3_range refuses its range once per packing: the kernel would carry an
    infinity on in silence"""
    with torch.no_grad():
        ok = torch.stack([torch.isfinite(_lp_fragments(p, kind, c_out, precision)).all() for p, (kind, c_out, _) in zip(packs, layers)])
        for good, (_, _, name) in zip(ok.cpu().tolist(), layers):
            if not good:
                raise ValueError(f"precision {precision!r}: a folded weight of {name or 'the layer'} is not finite as {precision}"
                                 + (f" (fp16's range ends at {_hip.F16_MAX:g})" if precision == "fp16" else "")
                                 + "; this layer cannot run on 16-bit operands (use precision 'fp32' or 'bf16')")


def pack_layer(conv, bn, kind, precision="fp32", name=None, check=True):
    """fold and pack one layer -> a device tensor: float32 (dal3_conv2d_pack), or for 'fp16' / 'bf16' the uint8 blob of
    dal3_conv2d_lp_pack. `name`: what a refusal calls the layer; check=False leaves refuse_nonfinite_weights to the caller,
    who packs several layers and checks them with one synchronisation."""
    dtype = check_precision(precision)
    L = _hip.fold_layer_struct(conv, bn)
    lib, eps = _hip.lib(), float(bn.eps) if bn is not None else 1e-5
    if precision == "fp32":
        buf = torch.empty(lib.dal3_conv2d_pack_floats(kind, L.c_in, L.c_out), dtype=torch.float32, device=conv.weight.device)
        _hip.check(lib.dal3_conv2d_pack(L, kind, eps, _hip.ptr(buf), _hip.stream()))
        return buf
    buf = torch.empty(lib.dal3_conv2d_lp_pack_bytes(kind, L.c_in, L.c_out), dtype=torch.uint8, device=conv.weight.device)
    _hip.check(lib.dal3_conv2d_lp_pack(L, kind, eps, dtype, _hip.ptr(buf), _hip.stream()))
    if check:
        refuse_nonfinite_weights([buf], [(kind, L.c_out, name)], precision)
    return buf


def out_size(kind, stride, H, W):
    if kind == _hip.CONV2D_3X3:
        return (H - 1) // stride + 1, (W - 1) // stride + 1
    if kind == _hip.CONV2D_1X1:
        return H, W
    return H * stride, W * stride


_nchw_map = _hip.nchw_map


def conv2d(x, packed, kind, stride, relu, c_out, out=None, channel_offset=0, max_workgroups=0, precision="fp32"):
    """one layer: x (B, c_in, H, W) float32 CUDA, any strides -> channels [channel_offset, channel_offset + c_out) of `out`
    (B, >= channel_offset + c_out, OH, OW) (allocated when None), returned as a view. Enqueued on the current stream.
    `precision`: what `packed` was packed as ('fp16' / 'bf16': dal3_conv2d_lp; x and out stay float32)."""
    dtype = check_precision(precision)
    if not torch.is_tensor(x):
        raise TypeError("x must be a tensor")
    _hip.require_gpu(x, "x")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"x must be float32 (B, C, H, W), got {x.dtype} {tuple(x.shape)}")
    B, c_in, H, W = x.shape
    OH, OW = out_size(kind, stride, H, W)
    if out is None:
        out = torch.empty((B, channel_offset + c_out, OH, OW), dtype=torch.float32, device=x.device)
    else:
        _hip.require_gpu(out, "out")
        if out.dtype != torch.float32 or out.dim() != 4 or out.shape[0] != B or tuple(out.shape[2:]) != (OH, OW) or out.device != x.device:
            raise ValueError(f"out must be float32 ({B}, channels, {OH}, {OW}) on {x.device}, got {out.dtype} {tuple(out.shape)}")
    lib, lp = _hip.lib(), precision != "fp32"
    want = lib.dal3_conv2d_lp_pack_bytes(kind, c_in, c_out) if lp else lib.dal3_conv2d_pack_floats(kind, c_in, c_out)
    if packed.dtype != (torch.uint8 if lp else torch.float32) or packed.numel() != want or packed.device != x.device:
        raise ValueError(f"the packed weights are not those of a {c_in} -> {c_out} layer of kind {kind} in {precision} on {x.device}")
    fields = dict(kind=kind, stride=stride, relu=1 if relu else 0, c_in=c_in, c_out=c_out, y_channels=out.shape[1],
                  y_channel_offset=channel_offset, max_workgroups=int(max_workgroups), B=B, H=H, W=W, x=_nchw_map(x),
                  y=_nchw_map(out), packed=_hip.ptr(packed))
    if B and H and W:
        if lp:
            _hip.check(lib.dal3_conv2d_lp(_hip.Conv2dLpArgs(dtype=dtype, **fields), _hip.stream()))
        else:
            _hip.check(lib.dal3_conv2d(_hip.Conv2dArgs(**fields), _hip.stream()))
    return out[:, channel_offset:channel_offset + c_out]


# ------------------------------------------------------------------------------------- training: the backward pass
_DECONVS = (_hip.CONV2D_DECONV2, _hip.CONV2D_DECONV4)


def layer_widths(weight, kind):
    """(c_in, c_out) of a Conv2d's (c_out, c_in, k, k) or a ConvTranspose2d's (c_in, c_out, s, s) weight"""
    return (weight.shape[0], weight.shape[1]) if kind in _DECONVS else (weight.shape[1], weight.shape[0])


def _check_map(t, what, shape=None):
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor")
    _hip.require_gpu(t, what)
    if t.dim() != 4 or t.dtype != torch.float32 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{what} must be float32 {'(B, C, H, W)' if shape is None else tuple(shape)}, got {t.dtype} {tuple(t.shape)}")


def pack_raw(weight, bias, kind, c_in, c_out):
    """dal3_conv2d_pack without a fold: a contiguous float32 weight of c_in -> c_out in the form's own layout, its bias or None"""
    for t in (weight, bias):
        if t is not None:
            _hip.require_gpu(t, "the layer's parameters")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("weights must be contiguous fp32")
    lib = _hip.lib()
    L = _hip.Layer(_hip.ptr(weight), _hip.ptr(bias), None, None, None, None, c_in, c_out)
    buf = torch.empty(lib.dal3_conv2d_pack_floats(kind, c_in, c_out), dtype=torch.float32, device=weight.device)
    _hip.check(lib.dal3_conv2d_pack(L, kind, 1e-5, _hip.ptr(buf), _hip.stream()))
    return buf


def conv2d_dgrad(dy, weight, kind, stride, in_size, out=None, max_workgroups=0):
    """the data gradient of one layer: dy (B, c_out, OH, OW) float32 CUDA of any strides and the layer's weight -> dx
    (B, c_in, H, W), in_size = (H, W) (a stride-2 layer's output does not determine it). `out`: a (B, c_in, H, W) view to
    write (allocated with torch.empty when None; every element is written). 3x3 of stride 1 and 1x1 are dal3_conv2d on the
    transposed pack; 3x3 of stride 2 and the transposed convolutions are dal3_conv2d_dgrad. Enqueued on the current stream."""
    c_in, c_out = layer_widths(weight, kind)
    H, W = in_size
    B = dy.shape[0] if torch.is_tensor(dy) and dy.dim() == 4 else 0
    _check_map(dy, "dy", (B, c_out, *out_size(kind, stride, H, W)))
    if out is None:
        out = torch.empty((B, c_in, H, W), dtype=torch.float32, device=dy.device)
    _check_map(out, "out", (B, c_in, H, W))
    w = weight.detach()
    if kind == _hip.CONV2D_1X1 or (kind == _hip.CONV2D_3X3 and stride == 1):
        wt = (w.flip(2, 3) if kind == _hip.CONV2D_3X3 else w).transpose(0, 1).contiguous()
        conv2d(dy, pack_raw(wt, None, kind, c_out, c_in), kind, 1, False, c_in, out=out, max_workgroups=max_workgroups)
        return out
    lib = _hip.lib()
    w = w.contiguous()
    _hip.require_gpu(w, "the layer's weight")
    packed = torch.empty(lib.dal3_conv2d_dgrad_pack_floats(kind, c_in, c_out), dtype=torch.float32, device=dy.device)
    _hip.check(lib.dal3_conv2d_dgrad_pack(_hip.ptr(w), kind, c_in, c_out, _hip.ptr(packed), _hip.stream()))
    if B and H and W:
        a = _hip.Conv2dDgradArgs(kind=kind, stride=stride, c_in=c_in, c_out=c_out, max_workgroups=int(max_workgroups), B=B, H=H, W=W,
                                 dy=_nchw_map(dy), dx=_nchw_map(out), packed=_hip.ptr(packed))
        _hip.check(lib.dal3_conv2d_dgrad(a, _hip.stream()))
    return out


def conv2d_wgrad_workspace_bytes(kind, stride, c_in, c_out, B, H, W):
    return _hip.lib().dal3_conv2d_wgrad_workspace_bytes(kind, stride, c_in, c_out, B, H, W)


def conv2d_wgrad(x, dy, kind, stride, weight_shape, bias=True, dw=None, db=None, max_workgroups=0):
    """one dal3_conv2d_wgrad call: the layer's input x (B, c_in, H, W) and the incoming gradient dy (B, c_out, OH, OW), float32
    CUDA of any strides -> (dW in the parameter's own layout, db (c_out) or None). `dw` / `db`: contiguous tensors to write
    (allocated when None)."""
    weight_shape = tuple(weight_shape)
    c_in, c_out = (weight_shape[0], weight_shape[1]) if kind in _DECONVS else (weight_shape[1], weight_shape[0])
    _check_map(x, "x")
    B, _, H, W = x.shape
    _check_map(x, "x", (B, c_in, H, W))
    _check_map(dy, "dy", (B, c_out, *out_size(kind, stride, H, W)))
    dev, lib = x.device, _hip.lib()
    if dw is None:
        dw = torch.empty(weight_shape, dtype=torch.float32, device=dev)
    if db is None and bias:
        db = torch.empty(c_out, dtype=torch.float32, device=dev)
    for t, shape in ((dw, weight_shape), (db, (c_out,))):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape or t.device != dev):
            raise ValueError(f"a gradient buffer must be contiguous float32 {shape} on {dev}, got {t.dtype} {tuple(t.shape)}")
    nbytes = lib.dal3_conv2d_wgrad_workspace_bytes(kind, stride, c_in, c_out, B, H, W)
    ws = _hip.workspace(nbytes, dev)
    a = _hip.Conv2dWgradArgs(kind=kind, stride=stride, c_in=c_in, c_out=c_out, max_workgroups=int(max_workgroups), B=B, H=H, W=W,
                             x=_nchw_map(x), dy=_nchw_map(dy), dw=_hip.ptr(dw), db=_hip.ptr(db if bias else None),
                             workspace=_hip.ptr(ws), workspace_bytes=nbytes)
    _hip.check(lib.dal3_conv2d_wgrad(a, _hip.stream()))
    return dw, (db if bias else None)


class _Conv2dFunction(torch.autograd.Function):
    """y = dal3_conv2d(x; weight, bias) on the raw pack (no fold, no ReLU). The backward: dx by the form's route
    (conv2d_dgrad), (dW, db) through dal3_conv2d_wgrad; each is skipped when nothing asks for it. The maps are read through
    their strides, nothing synchronises and everything is enqueued on the current stream."""

    @staticmethod
    def forward(ctx, x, weight, bias, kind, stride, max_workgroups):
        c_in, c_out = layer_widths(weight, kind)
        packed = pack_raw(weight.detach(), None if bias is None else bias.detach(), kind, c_in, c_out)
        y = conv2d(x, packed, kind, stride, False, c_out, max_workgroups=max_workgroups)
        ctx.save_for_backward(x, weight)
        ctx.form, ctx.has_bias = (kind, stride, max_workgroups), bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        kind, stride, mw = ctx.form
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = conv2d_dgrad(dy, weight, kind, stride, x.shape[2:], max_workgroups=mw)
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_db:
            dw, db = conv2d_wgrad(x, dy, kind, stride, weight.shape, bias=want_db, max_workgroups=mw)
        return dx, dw, db, None, None, None


def conv2d_train(x, conv, max_workgroups=0):
    """an nn.Conv2d / nn.ConvTranspose2d that dal3_conv2d serves (layer_kind), differentiable on the HIP kernels"""
    form = layer_kind(conv)
    if form is None:
        raise NotImplementedError(f"{conv}: dal3_conv2d serves Conv 3x3 of stride 1 or 2, Conv 1x1 and ConvTranspose k = s in (2, 4)")
    return _Conv2dFunction.apply(x, conv.weight, conv.bias, form[0], form[1], int(max_workgroups))


def _train_sequence(seq, x, max_workgroups):
    """a reference Sequential in training: every convolution through _Conv2dFunction (which pads a 3x3 itself: a
    ZeroPad2d in front of it is skipped, as `_split` does), every norm layer as the stock module, ReLU stock"""
    for m in seq:
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            x = conv2d_train(x, m, max_workgroups)
        elif isinstance(m, nn.ReLU):
            x = torch.relu(x)
        elif not isinstance(m, nn.ZeroPad2d):
            x = m(x)
    return x


def _refuse_train_forward(module, sequences, x):
    """what `train_forward` refuses, in words"""
    name = type(module).__name__
    for seq in sequences:
        for _, bn, _ in _split(seq):
            if not _norm_ok(bn):
                raise NotImplementedError(f"{name}.train_forward: the norm layer {bn} is not an affine nn.BatchNorm2d with running statistics")
    if not module.hip_serves():
        raise NotImplementedError(f"{name}.train_forward: this configuration has a layer that dal3_conv2d does not serve (hip_serves() is "
                                  "False): train it through composite()")
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"{name}.train_forward runs only on the GPU through lib3dal_hip.so (x lives on "
                           f"{x.device if torch.is_tensor(x) else type(x).__name__}); composite() is the stock-torch route")


def conv2d_flop(kind, stride, c_in, c_out, H, W, B=1):
    """(algorithmic, executed) FLOP of one layer: 2 * MACs from the shapes, and what the kernel's tiles (32 GEMM rows,
    8 x 32 pixels, 8 input channels) execute"""
    taps, sub = KIND_TAPS[kind], KIND_SUB[kind]
    ph, pw = out_size(kind, stride, H, W) if kind == _hip.CONV2D_3X3 else (H, W)
    algo = 2 * B * ph * pw * c_out * sub * c_in * taps
    rows, k, up = -(-c_out * sub // 32) * 32, -(-c_in // 8) * 8, lambda v, m: -(-v // m) * m
    return algo, 2 * B * up(ph, 8) * up(pw, 32) * rows * k * taps


def conv2d_lp_flop(kind, stride, c_in, c_out, H, W, B=1):
    """conv2d_flop for the 16-bit kernel, whose tiles differ in one extent: 16 input channels a k-step, not 8"""
    taps, sub = KIND_TAPS[kind], KIND_SUB[kind]
    ph, pw = out_size(kind, stride, H, W) if kind == _hip.CONV2D_3X3 else (H, W)
    rows, k, up = -(-c_out * sub // 32) * 32, -(-c_in // 16) * 16, lambda v, m: -(-v // m) * m
    return conv2d_flop(kind, stride, c_in, c_out, H, W, B)[0], 2 * B * up(ph, 8) * up(pw, 32) * rows * k * taps


class _PackedLayers(nn.Module):
    """the packed-weights cache of a module whose `_plan()` lists its kernel layers as (conv, bn, kind, stride, relu);
    `_pack_key()` is whatever else the pack depends on"""

    def __init__(self):
        super().__init__()
        self._packed, self._stamp = None, None

    def _pack_key(self):
        return None

    def invalidate_packed(self):
        """after writes that bypass the tensors' version counters (`.data` writes, raw pointers)"""
        self._packed, self._stamp = None, None

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self.invalidate_packed()
        return out

    def train(self, mode=True):
        out = super().train(mode)
        self.invalidate_packed()
        return out

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self.invalidate_packed()
        return out

    def packed(self):
        plan = self._plan()
        ts = [t for conv, bn, *_ in plan for t in list(conv.parameters()) + (list(bn.parameters()) + list(bn.buffers()) if bn is not None else [])]
        stamp = (self._pack_key(), tuple((t.data_ptr(), t._version, t.device) for t in ts))
        if self._packed is None or stamp != self._stamp:
            self._packed, self._stamp = self._pack(plan), stamp
        return self._packed

    def _pack(self, plan):
        return [pack_layer(conv, bn, kind) for conv, bn, kind, _, _ in plan]


class _DenseLayers(_PackedLayers):
    """_PackedLayers of the dense stage's two modules. `precision` ('fp32', the default, | 'fp16' | 'bf16') is the MFMA
    operand type of the eval-mode kernel route; it is part of the cache's key, so changing it repacks. Train mode and a
    module the kernel does not serve run the composite, whatever it says."""

    def __init__(self):
        super().__init__()
        self._precision = "fp32"

    @property
    def precision(self):
        return self._precision

    @precision.setter
    def precision(self, value):
        check_precision(value)
        self._precision = value

    def _pack_key(self):
        return self._precision

    def _pack(self, plan):
        names = {m: n for n, m in self.named_modules()}
        packs = [pack_layer(conv, bn, kind, self._precision, names.get(conv), check=False) for conv, bn, kind, _, _ in plan]
        if self._precision != "fp32":
            refuse_nonfinite_weights(packs, [(kind, conv.out_channels, names.get(conv)) for conv, _, kind, _, _ in plan], self._precision)
        return packs


def _split(seq):
    """a reference Sequential -> [(conv, norm or None, relu)] by position; padding modules are skipped"""
    out = []
    for m in seq:
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            out.append([m, None, False])
        elif isinstance(m, nn.ReLU):
            out[-1][2] = True
        elif not isinstance(m, nn.ZeroPad2d):
            out[-1][1] = m
    return out


class RPN(_DenseLayers):
    """det3d/models/necks/rpn.py. forward(x (B, num_input_features, H, W)) -> (B, sum(us_num_filters), H', W')."""

    def __init__(self, layer_nums, ds_layer_strides, ds_num_filters, us_layer_strides, us_num_filters, num_input_features,
                 norm_cfg=None, name="rpn", logger=None, **kwargs):
        super().__init__()
        self._layer_strides, self._num_filters, self._layer_nums = ds_layer_strides, ds_num_filters, layer_nums
        self._upsample_strides, self._num_upsample_filters = us_layer_strides, us_num_filters
        self._num_input_features = num_input_features
        self._norm_cfg = dict(type="BN", eps=1e-3, momentum=0.01) if norm_cfg is None else norm_cfg
        assert len(self._layer_strides) == len(self._layer_nums) == len(self._num_filters)
        assert len(self._num_upsample_filters) == len(self._upsample_strides)
        self._upsample_start_idx = len(self._layer_nums) - len(self._upsample_strides)
        must_equal = [self._upsample_strides[i] / np.prod(self._layer_strides[:i + self._upsample_start_idx + 1])
                      for i in range(len(self._upsample_strides))]
        assert all(v == must_equal[0] for v in must_equal)
        in_filters = [num_input_features, *self._num_filters[:-1]]
        blocks, deblocks = [], []
        for i, layer_num in enumerate(self._layer_nums):
            planes = self._num_filters[i]
            block = [nn.ZeroPad2d(1), nn.Conv2d(in_filters[i], planes, 3, stride=self._layer_strides[i], bias=False),
                     build_norm_layer(self._norm_cfg, planes), nn.ReLU()]
            for _ in range(layer_num):
                block += [nn.Conv2d(planes, planes, 3, padding=1, bias=False), build_norm_layer(self._norm_cfg, planes), nn.ReLU()]
            blocks.append(nn.Sequential(*block))
            j = i - self._upsample_start_idx
            if j >= 0:
                stride, up = self._upsample_strides[j], self._num_upsample_filters[j]
                if stride > 1:
                    conv = nn.ConvTranspose2d(planes, up, stride, stride=stride, bias=False)
                else:
                    stride = int(np.round(1 / stride))
                    conv = nn.Conv2d(planes, up, stride, stride=stride, bias=False)
                deblocks.append(nn.Sequential(conv, build_norm_layer(self._norm_cfg, up), nn.ReLU()))
        self.blocks = nn.ModuleList(blocks)
        self.deblocks = nn.ModuleList(deblocks)
        if logger is not None:
            logger.info("Finish RPN Initialization")

    @property
    def downsample_factor(self):
        factor = np.prod(self._layer_strides)
        if len(self._upsample_strides) > 0:
            factor /= self._upsample_strides[-1]
        return factor

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight)

    def _plan(self):
        """[(conv, bn, kind, stride, relu)]: every block's layers, then every deblock's"""
        return [(conv, bn, *layer_kind(conv), relu) for seq in list(self.blocks) + list(self.deblocks) for conv, bn, relu in _split(seq)]

    def hip_serves(self):
        """whether the eval-mode forward of this module runs the HIP kernel"""
        for seq in list(self.blocks) + list(self.deblocks):
            for conv, bn, _ in _split(seq):
                kind = layer_kind(conv)
                if kind is None or not _norm_ok(bn) or (kind[0] == _hip.CONV2D_3X3 and conv.padding not in ((0, 0), (1, 1))):
                    return False
        return len(self.deblocks) > 0

    def composite(self, x):
        """the same definition in stock torch ops (the reference's forward); differentiable, BatchNorm by its mode"""
        ups = []
        for i, block in enumerate(self.blocks):
            x = block(x)
            if i - self._upsample_start_idx >= 0:
                ups.append(self.deblocks[i - self._upsample_start_idx](x))
        return torch.cat(ups, dim=1) if ups else x

    def train_forward(self, x, max_workgroups=0):
        """composite()'s graph with every convolution on the HIP kernels (_Conv2dFunction: dal3_conv2d forward, the data and
        weight gradients of dal3_conv2d_dgrad / dal3_conv2d_wgrad), float32 whatever `precision` says. Every norm layer is
        called as the stock module, so it acts by its own mode (batch statistics and running-stat updates in train mode,
        the running statistics when frozen); ReLU and torch.cat are stock. Refuses, in words, a configuration that
        hip_serves() refuses, a norm layer that is no affine nn.BatchNorm2d with running statistics, and a CPU tensor."""
        _refuse_train_forward(self, list(self.blocks) + list(self.deblocks), x)
        ups = []
        for i, block in enumerate(self.blocks):
            x = _train_sequence(block, x, max_workgroups)
            if i - self._upsample_start_idx >= 0:
                ups.append(_train_sequence(self.deblocks[i - self._upsample_start_idx], x, max_workgroups))
        return torch.cat(ups, dim=1)

    def forward(self, x, max_workgroups=0):
        if self.training or not self.hip_serves():
            return self.composite(x)
        with torch.no_grad():
            packed, plan, prec = self.packed(), self._plan(), self._precision
            at, n_block_layers = 0, sum(len(_split(b)) for b in self.blocks)
            ups, offset, out = [], 0, None
            for i, block in enumerate(self.blocks):
                for _ in _split(block):
                    conv, _, kind, stride, relu = plan[at]
                    x = conv2d(x, packed[at], kind, stride, relu, conv.out_channels, max_workgroups=max_workgroups, precision=prec)
                    at += 1
                j = i - self._upsample_start_idx
                if j >= 0:
                    conv, _, kind, stride, relu = plan[n_block_layers + j]
                    size = out_size(kind, stride, x.shape[2], x.shape[3])
                    if out is None:
                        out = torch.empty((x.shape[0], sum(self._num_upsample_filters), *size), dtype=torch.float32, device=x.device)
                    elif tuple(out.shape[2:]) != size:
                        raise RuntimeError(f"the upsampled maps differ in size ({tuple(out.shape[2:])} and {size}): torch.cat would refuse them")
                    conv2d(x, packed[n_block_layers + j], kind, stride, relu, conv.out_channels, out=out, channel_offset=offset,
                           max_workgroups=max_workgroups, precision=prec)
                    offset += conv.out_channels
            return out


class SepHead(nn.Module):
    """center_head.py:65-110: one Sequential per head, [Conv, (BatchNorm2d), ReLU] * (num_conv - 1) + [Conv]. A parameter
    container with the reference's forward; CenterHead runs its layers through the kernel."""

    def __init__(self, in_channels, heads, head_conv=64, final_kernel=1, bn=False, init_bias=-2.19, **kwargs):
        super().__init__(**kwargs)
        self.heads = heads
        for head in self.heads:
            classes, num_conv = self.heads[head]
            fc = []
            for _ in range(num_conv - 1):
                fc.append(nn.Conv2d(in_channels, head_conv, kernel_size=final_kernel, stride=1, padding=final_kernel // 2, bias=True))
                if bn:
                    fc.append(nn.BatchNorm2d(head_conv))
                fc.append(nn.ReLU())
            fc.append(nn.Conv2d(head_conv, classes, kernel_size=final_kernel, stride=1, padding=final_kernel // 2, bias=True))
            fc = nn.Sequential(*fc)
            if "hm" in head:
                fc[-1].bias.data.fill_(init_bias)
            else:
                for m in fc.modules():
                    if isinstance(m, nn.Conv2d):
                        nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                        nn.init.constant_(m.bias, 0)
            self.__setattr__(head, fc)

    def forward(self, x):
        return {head: self.__getattr__(head)(x) for head in self.heads}


class CenterHead(_DenseLayers):
    """center_head.py:167-244 and `predict` (through detect.CenterHeadPost). forward(x) -> one dict per task of logical
    (B, c, H, W) maps; on the kernel route they are channel slices of one tensor per task."""

    def __init__(self, in_channels=[128, ], tasks=[], dataset="nuscenes", weight=0.25, code_weights=[], common_heads=dict(),
                 logger=None, init_bias=-2.19, share_conv_channel=64, num_hm_conv=2, dcn_head=False):
        super().__init__()
        if dcn_head:
            raise NotImplementedError("dcn_head=True (deformable convolutions in the head) is not supported")
        num_classes = [len(t["class_names"]) for t in tasks]
        self.class_names = [t["class_names"] for t in tasks]
        self.code_weights, self.weight, self.dataset = code_weights, weight, dataset
        self.in_channels, self.num_classes = in_channels, num_classes
        self.box_n_dim = 9 if "vel" in common_heads else 7
        self.use_direction_classifier = False
        self.shared_conv = nn.Sequential(nn.Conv2d(in_channels, share_conv_channel, kernel_size=3, padding=1, bias=True),
                                         nn.BatchNorm2d(share_conv_channel), nn.ReLU(inplace=True))
        self.tasks = nn.ModuleList()
        for num_cls in num_classes:
            heads = copy.deepcopy(common_heads)
            heads.update(dict(hm=(num_cls, num_hm_conv)))
            self.tasks.append(SepHead(share_conv_channel, heads, bn=True, init_bias=init_bias, final_kernel=3))
        self._post = None

    def _sequences(self):
        return [self.shared_conv] + [getattr(task, head) for task in self.tasks for head in task.heads]

    def _plan(self):
        return [(conv, bn, *layer_kind(conv), relu) for seq in self._sequences() for conv, bn, relu in _split(seq)]

    def hip_serves(self):
        """whether the eval-mode forward of this module runs the HIP kernel"""
        for seq in self._sequences():
            for conv, bn, _ in _split(seq):
                kind = layer_kind(conv)
                if kind is None or not _norm_ok(bn) or (kind[0] == _hip.CONV2D_3X3 and conv.padding != (1, 1)):
                    return False
        return True

    def _fusable(self, task):
        """the first convolutions of a task's heads read the same input: they run as one launch when each is one 3x3
        layer of a multiple of 64 channels (whole row groups of the kernel), which leaves every output's k-order as it is
        when run alone"""
        firsts = [_split(getattr(task, head)) for head in task.heads]
        return all(len(f) == 2 and f[0][0].out_channels % 64 == 0 and f[0][0].kernel_size == (3, 3) for f in firsts)

    def _pack(self, plan):
        packs = super()._pack(plan)
        fused, at = [], 1
        for task in self.tasks:
            n = [len(_split(getattr(task, head))) for head in task.heads]
            if self._fusable(task):
                first = [packs[at + sum(n[:i])] for i in range(len(n))]
                rows = [plan[at + sum(n[:i])][0].out_channels for i in range(len(n))]
                # a pack is [bias of every GEMM row | fragments by out tile]: the fused layer's is both parts concatenated
                # (a 16-bit pack is a byte blob with the same two parts, its biases float32)
                rows = [r * (1 if self._precision == "fp32" else 4) for r in rows]
                fused.append(torch.cat([p[:r] for p, r in zip(first, rows)] + [p[r:] for p, r in zip(first, rows)]))
            else:
                fused.append(None)
            at += sum(n)
        return packs, fused

    def composite(self, x):
        """the same definition in stock torch ops (the reference's forward)"""
        x = self.shared_conv(x)
        return [task(x) for task in self.tasks]

    def train_forward(self, x, max_workgroups=0):
        """composite()'s graph with every convolution on the HIP kernels (RPN.train_forward's contract and refusals) -> one
        dict per task of (B, c, H, W) maps. The heads' first layers are not fused in training: each is a launch of its own."""
        _refuse_train_forward(self, self._sequences(), x)
        x = _train_sequence(self.shared_conv, x, max_workgroups)
        return [{head: _train_sequence(getattr(task, head), x, max_workgroups) for head in task.heads} for task in self.tasks]

    def forward(self, x, *kwargs, max_workgroups=0):
        if self.training or not self.hip_serves():
            return self.composite(x)
        with torch.no_grad():
            (packed, fused), plan, prec = self.packed(), self._plan(), self._precision

            def run(at, x, **kw):
                conv, _, kind, stride, relu = plan[at]
                return conv2d(x, packed[at], kind, stride, relu, conv.out_channels, max_workgroups=max_workgroups, precision=prec, **kw)

            x = run(0, x)
            at, ret = 1, []
            for t, task in enumerate(self.tasks):
                n = [len(_split(getattr(task, head))) for head in task.heads]
                classes = [task.heads[head][0] for head in task.heads]
                maps = torch.empty((x.shape[0], sum(classes), x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
                mid = None
                if fused[t] is not None:
                    widths = [plan[at + sum(n[:i])][0].out_channels for i in range(len(n))]
                    mid = conv2d(x, fused[t], _hip.CONV2D_3X3, 1, True, sum(widths), max_workgroups=max_workgroups, precision=prec)
                d, offset = {}, 0
                for i, head in enumerate(task.heads):
                    y = x
                    if mid is not None:
                        y = mid[:, sum(widths[:i]):sum(widths[:i + 1])]
                        at += 1
                    for k in range(n[i] - (1 if mid is None else 2)):
                        y = run(at, y)
                        at += 1
                    d[head] = run(at, y, out=maps, channel_offset=offset)
                    at += 1
                    offset += classes[i]
                ret.append(d)
            return ret

    def _loss_heads(self, preds_dict):
        """what `loss` serves, refused in words otherwise -> the number of regression columns"""
        from . import center_loss
        if self.dataset not in ("waymo", "nuscenes"):
            raise NotImplementedError(f"dataset {self.dataset!r}: the loss is built for 'waymo' and 'nuscenes' (the reference "
                                      "raises for every other one)")
        if len(self.code_weights) == 0:
            raise ValueError("code_weights is empty: the loss needs one weight per regression column (8, or 10 with vel)")
        heads = set(preds_dict)
        if "hm" not in heads or not {"reg", "height", "dim", "rot"} <= heads or not heads <= {"hm", *center_loss.REG_HEADS}:
            raise NotImplementedError(f"heads {sorted(heads)}: the loss is built for hm, reg, height, dim, rot and an optional vel")
        n_cols = 10 if "vel" in heads else 8
        if len(self.code_weights) != n_cols:
            raise ValueError(f"code_weights has {len(self.code_weights)} entries, the heads make {n_cols} regression columns")
        return n_cols

    def loss(self, example, preds_dicts, **kwargs):
        """center_head.py's loss: example holds the lists hm, anno_box, ind, mask, cat (center_loss.center_targets makes
        them), preds_dicts is forward's list -> the merged dictionary of lists loss, hm_loss, loc_loss, loc_loss_elem,
        num_positive, one entry per task. One dal3_center_loss call per task reads the raw maps in place (the kernel
        route's channel slices as well as the composite route's tensors) and yields the gradients with the loss; `loss`
        carries the graph, the other entries are detached, as the reference's hm_loss and loc_loss_elem are.
        Differences from the reference: every value stays a device tensor and nothing is read back (the reference's
        .detach().cpu() is a host synchronisation per task); preds_dicts is not changed (no in-place sigmoid, no
        anno_box key); and `loc_loss`, which the reference returns with its graph, is returned detached: the gradients
        the kernel writes are those of `loss`, so backward goes through `loss` alone."""
        from . import center_loss
        merged = {k: [] for k in ("loss", "hm_loss", "loc_loss", "loc_loss_elem", "num_positive")}
        if len(preds_dicts) != len(self.tasks):
            raise ValueError(f"{len(preds_dicts)} prediction dictionaries for {len(self.tasks)} tasks")
        for t, preds in enumerate(preds_dicts):
            self._loss_heads(preds)
            vals = center_loss.head_loss(preds, example["hm"][t], example["anno_box"][t], example["ind"][t], example["mask"][t],
                                         example["cat"][t], self.code_weights, self.weight)
            for k, v in zip(merged, vals):
                merged[k].append(v)
        return merged

    def loss_from_gt(self, preds_dicts, gt_boxes_and_cls, assigner, voxels=None):
        """targets and loss chained on the current stream: `assigner` is a center_loss.AssignLabel (`voxels`: the
        voxeliser's entry, when the assigner was built without it) -> loss(...)'s dictionary"""
        return self.loss(assigner(gt_boxes_and_cls, voxels), preds_dicts)

    @torch.no_grad()
    def predict(self, example, preds_dicts, test_cfg, **kwargs):
        """center_head.py:294 through detect.CenterHeadPost, or detect.DoubleFlipPost when test_cfg has double_flip (the batch
        then holds four views per sample) -> the per-sample list of box3d_lidar / scores / label_preds / metadata; one host
        synchronisation"""
        from . import detect
        if self._post is None or self._post[0] is not test_cfg:
            post = detect.DoubleFlipPost if detect._get(test_cfg, "double_flip", False) else detect.CenterHeadPost
            self._post = (test_cfg, post(test_cfg, self.num_classes))
        meta = example.get("metadata") if isinstance(example, dict) else None
        return self._post[1].predict(preds_dicts, metadata=meta)
