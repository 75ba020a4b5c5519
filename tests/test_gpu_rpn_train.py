"""The dense stage's training route on the GPU (3dal_pytorch_amd/rpn.py: _Conv2dFunction, RPN.train_forward,
CenterHead.train_forward; dal3_conv2d_dgrad / dal3_conv2d_wgrad): impulses pin the data gradient's taps, phases and
sub-positions and the weight gradient's taps, border and bias sum bit for bit, inside sentinel-filled buffers; single
layers, the slice seam, the whole neck and head and VoxelNet.first_stage_loss(dense="hip") are judged against the float64
autograd truth of tests/rpn_train_ref.py with torch-CPU fp32 autograd as the yardstick, under rpn_train_ref.BARS. The
shapes are the smallest that cross each seam: dgrad's 8 x 32 pixel tile (a stride-2 phase's is 16 x 64 pixels of dx) and
16-channel chunk, wgrad's 4 x 32 (4 x 16 for the stride-4 transposed convolution) pixel tile, its 32 x 32 channel tile
and its slice of DAL3_CONV2D_WGRAD_SLICE pixels.

With DAL3_RPN_TRAIN_RECORD=<path> in the environment the run also writes every measure, yardstick and ratio to <path>
(how profiles/rpn_train_measured.json was made)."""
import functools
import importlib
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import rpn_ref as R
import rpn_train_ref as T
from rpn_gpu import KINDS, _dev, head_module, neck_module
from rpn_gpu import _hold as _hold_forward

hip = importlib.import_module("3dal_pytorch_amd._hip")
rpn = importlib.import_module("3dal_pytorch_amd.rpn")
pytestmark = pytest.mark.gpu

IMPULSE = dict(B=2, c_in=24, c_out=40, H=11, W=37, offset=3, channels=50)      # test_gpu_rpn.IMPULSE
SENTINEL = -7.5
_RECORD = {}


@pytest.fixture(autouse=True)
def _grad_on():
    """whatever a test before this file left switched"""
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    path = os.environ.get("DAL3_RPN_TRAIN_RECORD")
    if path and _RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        # one line a row, four significant digits: [measured, yardstick, ratio], each in the order of `measures`
        sig = lambda d: [float(f"{d[k]:.4g}") for k in T.MEASURES]
        rows = ",\n".join(f' {json.dumps(k)}: {json.dumps([sig(v["measured"]), sig(v["yardstick"]), sig(v["ratio"])])}'
                          for k, v in sorted(_RECORD.items()))
        with open(path, "w") as f:
            f.write('{"measures": %s, "columns": ["measured", "yardstick", "ratio"], "rows": {\n%s\n}}\n' % (json.dumps(list(T.MEASURES)), rows))


def _hold(row, got, f32, truth, what="map", kind=None):
    """each measure <= bar x the fp32 yardstick's own error against the truth, dead channels +0"""
    ratio, m, y = T.ratios(got, f32, truth, what, kind)
    _RECORD[row] = {"measured": {k: m[k] for k in T.MEASURES}, "yardstick": {k: y[k] for k in T.MEASURES}, "ratio": ratio}
    for k in T.MEASURES:
        print(f"{row:44s} {k:9s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:7.2f}  bar {T.BARS[k]:g}")
    assert m["dead_ok"], row
    bad = [(k, m[k], ratio[k]) for k in T.MEASURES if ratio[k] > T.BARS[k]]
    assert not bad, (row, bad)


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).view(np.uint32)


def _spots(H, W):
    """test_gpu_rpn's spots on an (H, W) extent: corners, edges, the interior, and either side of the tile seams that fit"""
    s = [(y, x) for y in (0, H // 2, H - 1) for x in (0, W // 2, W - 1)]
    s += [p for p in ((7, 31), (8, 32), (3, 15), (4, 16), (15, 63), (16, 64)) if p[0] < H and p[1] < W]
    return list(dict.fromkeys(s))


def _weight(tag, kind, stride):
    I = IMPULSE
    return T.layer_case(tag, kind, stride, I["c_in"], I["c_out"], 1, 2, 2)[1]


# ------------------------------------------------------------------------------------- impulses, bit for bit
@pytest.mark.parametrize("kind,stride", T.FORMS)
def test_dgrad_impulses_are_bit_exact(kind, stride):
    I = IMPULSE
    B, H, W = I["B"], I["H"], I["W"]
    w = _weight(f"train/impulse/{kind}{stride}", kind, stride)
    wd = _dev(w)
    OH, OW = T.out_size(kind, stride, H, W)
    v = np.float32(0.7)
    dy = torch.zeros((B, I["c_out"], OH, OW), device="cuda")
    n = 0
    for b0 in range(B):
        for c0 in (0, I["c_out"] - 1):
            for y0, x0 in _spots(OH, OW):
                dy.zero_()
                dy[b0, c0, y0, x0] = float(v)
                ref = np.zeros((B, I["c_out"], OH, OW), np.float32)
                ref[b0, c0, y0, x0] = v
                # one term per element: the float64 product of two float32 values is exact, its rounding is fl32(W * v)
                want = T.dgrad_sum(ref, w, kind, stride, H, W).astype(np.float32)
                assert np.count_nonzero(want) >= I["c_in"] - 1 and not np.signbit(want[want == 0]).any()
                big = torch.full((B, I["channels"], H + 2, W + 3), SENTINEL, device="cuda")
                out = big[:, I["offset"]:I["offset"] + I["c_in"], 1:-1, 2:-1]
                got = rpn.conv2d_dgrad(dy, wd, KINDS[kind, stride], stride, (H, W), out=out, max_workgroups=n % 3)
                assert got.data_ptr() == out.data_ptr()
                assert np.array_equal(_bits(out), want.view(np.uint32)), (b0, c0, y0, x0)       # every element written, +0 elsewhere
                big[:, I["offset"]:I["offset"] + I["c_in"], 1:-1, 2:-1] = SENTINEL
                assert bool((big == SENTINEL).all()), "something outside the view was written"
                n += 1
    assert n >= 2 * 2 * 9


def _connected(kind, stride, y0, x0, OH, OW):
    """output pixels for the wgrad impulse at input (y0, x0): the pixel over it, a diagonal neighbour that reaches it through
    another tap (where the form has one), and a far pixel that no tap connects"""
    if kind == "deconv":
        near = [((y0 * stride, x0 * stride), "over"), ((y0 * stride + stride - 1, x0 * stride + 1), "diag")]
    elif kind == "1x1":
        near = [((y0, x0), "over")]
    else:
        oy, ox = y0 // stride, x0 // stride
        near = [((oy, ox), "over"), ((oy + 1 if oy + 1 < OH else oy - 1, ox - 1 if ox > 0 else ox + 1), "diag")]
    return near + [(((near[0][0][0] + OH // 2) % OH, near[0][0][1]), "far")]


@pytest.mark.parametrize("kind,stride", T.FORMS)
def test_wgrad_impulses_are_bit_exact(kind, stride):
    I = IMPULSE
    B, H, W, c_in, c_out = I["B"], I["H"], I["W"], I["c_in"], I["c_out"]
    shape = (c_in, c_out, stride, stride) if kind == "deconv" else (c_out, c_in, 3, 3) if kind == "3x3" else (c_out, c_in, 1, 1)
    n_w = int(np.prod(shape))
    OH, OW = T.out_size(kind, stride, H, W)
    a, v = np.float32(1.3), np.float32(0.7)
    x = torch.zeros((B, c_in, H, W), device="cuda")
    g = torch.zeros((B, c_out, OH, OW), device="cuda")
    n = hits = 0
    for b0 in range(B):
        for ci0, co0 in ((0, 0), (c_in - 1, c_out - 1)):
            for y0, x0 in _spots(H, W):
                for (oy, ox), role in _connected(kind, stride, y0, x0, OH, OW):
                    bg = b0 if role != "diag" or n % 4 else 1 - b0         # now and then the other batch item: nothing connects
                    x.zero_()
                    g.zero_()
                    x[b0, ci0, y0, x0] = float(a)
                    g[bg, co0, oy, ox] = float(v)
                    rx, rg = np.zeros((B, c_in, H, W), np.float32), np.zeros((B, c_out, OH, OW), np.float32)
                    rx[b0, ci0, y0, x0], rg[bg, co0, oy, ox] = a, v
                    want = T.wgrad_sum(rx, rg, kind, stride).astype(np.float32)
                    cnt = np.count_nonzero(want)
                    assert cnt == 1 if role == "over" else cnt == 0 if (role == "far" or bg != b0) else cnt <= 1
                    hits += cnt
                    if cnt:
                        assert want[want != 0][0] == np.float32(a * v)
                    want_db = np.zeros(c_out, np.float32)
                    want_db[co0] = v
                    buf = torch.full((n_w + c_out + 96,), SENTINEL, device="cuda")
                    dw, db = buf[32:32 + n_w].view(shape), buf[64 + n_w:64 + n_w + c_out]
                    rpn.conv2d_wgrad(x, g, KINDS[kind, stride], stride, shape, dw=dw, db=db, max_workgroups=n % 3)
                    got = buf.cpu().numpy()
                    assert np.array_equal(got[32:32 + n_w].view(np.uint32), want.reshape(-1).view(np.uint32)), (b0, ci0, y0, x0, oy, ox)
                    assert np.array_equal(got[64 + n_w:64 + n_w + c_out].view(np.uint32), want_db.view(np.uint32))
                    rest = np.concatenate([got[:32], got[32 + n_w:64 + n_w], got[64 + n_w + c_out:]])
                    assert (rest == SENTINEL).all(), "something outside dW and db was written"
                    n += 1
    assert hits >= n // 3
    # without db: NULL is accepted and dW has the same bits
    dw2, none = rpn.conv2d_wgrad(x, g, KINDS[kind, stride], stride, shape, bias=False)
    assert none is None and np.array_equal(_bits(dw2), _bits(dw))


# ------------------------------------------------------------------------------------- single layers against float64
PAIRS = ((64, 64), (128, 256), (384, 64), (64, 1), (64, 3))
# (canvas, B, kind, stride, view of x, view of dy, max_workgroups): every canvas, form, view and cap at least once per pair
SCHEDULE = (((5, 7), 2, "3x3", 1, "plain", "sliced", 0),
            ((12, 12), 1, "3x3", 2, "sliced", "channels_last", 1),
            ((13, 37), 2, "3x3", 2, "channels_last", "plain", 3),
            ((13, 37), 1, "3x3", 1, "sliced", "channels_last", 1),
            ((13, 37), 1, "1x1", 1, "channels_last", "sliced", 3),
            ((5, 7), 2, "deconv", 2, "sliced", "plain", 1),
            ((12, 12), 1, "deconv", 4, "plain", "channels_last", 0))


def _view(x, how):
    """test_gpu_rpn._view: the same values as a slice of a NaN-filled larger tensor, or in channels-last memory"""
    t = _dev(x)
    if how == "sliced":
        big = torch.full((t.shape[0], 2 * t.shape[1], t.shape[2] + 3, t.shape[3] + 5), float("nan"), device="cuda")
        big[:, ::2, 1:-2, 2:-3] = t
        t = big[:, ::2, 1:-2, 2:-3]
    elif how == "channels_last":
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert t.shape == x.shape
    return t


def _gpu_layer(x, w, b, cot, kind, stride, mw=0, x_view="plain", dy_view="plain"):
    """one layer through _Conv2dFunction -> (y, dx, dW, db) device tensors; x and the cotangent arrive behind the given strides"""
    xd = _view(x, x_view).requires_grad_()
    wd, bd = _dev(w).requires_grad_(), _dev(b).requires_grad_()
    y = rpn._Conv2dFunction.apply(xd, wd, bd, KINDS[kind, stride], stride, mw)
    dy = _view(cot, dy_view)
    # the gradient routes are called on the views themselves as well: autograd may hand backward() other strides
    dx_direct = rpn.conv2d_dgrad(dy, wd, KINDS[kind, stride], stride, x.shape[2:], max_workgroups=mw)
    dw_direct, db_direct = rpn.conv2d_wgrad(xd.detach(), dy, KINDS[kind, stride], stride, w.shape, max_workgroups=mw)
    y.backward(dy)
    for a, c in ((xd.grad, dx_direct), (wd.grad, dw_direct), (bd.grad, db_direct)):
        assert np.array_equal(_bits(a), _bits(c))
    return y.detach(), xd.grad, wd.grad, bd.grad


def _hold_layer(row, got, f32, truth, kind):
    k = "deconv" if kind == "deconv" else None
    for name, what in (("y", "map"), ("dx", "map"), ("dW", "weight"), ("db", "vector")):
        i = ("y", "dx", "dW", "db").index(name)
        _hold(f"{row}/{name}", got[i].cpu().numpy(), f32[i], truth[i], what, k)


@pytest.mark.parametrize("case", range(len(SCHEDULE)))
@pytest.mark.parametrize("c_in,c_out", PAIRS)
def test_single_layers_against_float64(c_in, c_out, case):
    (H, W), B, kind, stride, xv, dyv, mw = SCHEDULE[case]
    tag = f"train/layer/{c_in}-{c_out}/{kind}{stride}/{H}x{W}"
    x, w, b, cot = T.layer_case(tag, kind, stride, c_in, c_out, B, H, W)
    truth = T.layer_autograd(x, w, b, kind, stride, cot)
    f32 = T.layer_autograd(x, w, b, kind, stride, cot, torch.float32)
    got = _gpu_layer(x, w, b, cot, kind, stride, mw, xv, dyv)
    _hold_layer(tag + f"/wg{mw}", got, f32, truth, kind)


# ------------------------------------------------------------------------------------- the slice seam, the grid, the run
SEAM = dict(H=261, W=32)                        # 66 pixel tiles of 4 x 32: two whole slices of DAL3_CONV2D_WGRAD_SLICE pixels and two tiles
GRID_CASES = {"seam": ("3x3", 1, 16, 16, 1, SEAM["H"], SEAM["W"]), "stride2": ("3x3", 2, 40, 24, 2, 13, 37),
              "deconv4": ("deconv", 4, 24, 40, 2, 9, 21)}


@functools.lru_cache(maxsize=None)
def _grid_case(name):
    kind, stride, c_in, c_out, B, H, W = GRID_CASES[name]
    return T.layer_case(f"train/grid/{name}", kind, stride, c_in, c_out, B, H, W, occupied=1.0)


def test_slice_seam():
    kind, stride, c_in, c_out, B, H, W = GRID_CASES["seam"]
    assert 2 * hip.CONV2D_WGRAD_SLICE < B * H * W <= 2 * hip.CONV2D_WGRAD_SLICE + 256
    nbytes = rpn.conv2d_wgrad_workspace_bytes(KINDS[kind, stride], stride, c_in, c_out, B, H, W)
    assert nbytes == 3 * 4 * c_in * c_out * 9
    x, w, b, cot = _grid_case("seam")
    truth = T.layer_autograd(x, w, b, kind, stride, cot)
    f32 = T.layer_autograd(x, w, b, kind, stride, cot, torch.float32)
    _hold_layer("train/seam", _gpu_layer(x, w, b, cot, kind, stride), f32, truth, kind)
    # a value in the last, short slice alone reaches dW
    x1, c1 = np.zeros_like(x), np.zeros_like(cot)
    x1[0, 3, H - 1, 5], c1[0, 7, H - 1, 5] = 1.3, 0.7
    dw, db = rpn.conv2d_wgrad(_dev(x1), _dev(c1), KINDS[kind, stride], stride, w.shape)
    want = T.wgrad_sum(x1, c1, kind, stride).astype(np.float32)
    assert want[7, 3, 1, 1] == np.float32(np.float32(1.3) * np.float32(0.7)) and np.array_equal(_bits(dw), want.view(np.uint32))


@pytest.mark.parametrize("name", list(GRID_CASES))
def test_bits_do_not_depend_on_the_grid_or_the_run(name):
    kind, stride = GRID_CASES[name][:2]
    x, w, b, cot = _grid_case(name)
    runs = [_gpu_layer(x, w, b, cot, kind, stride, mw) for mw in (0, 0, 1, 3)]
    for other in runs[1:]:
        for a, c in zip(runs[0], other):
            assert np.array_equal(_bits(a), _bits(c))


def test_a_relu_dead_channel_has_plus_zero_gradients():
    c_in, c_out, dead = 24, 40, R.DEAD_CHANNEL
    x, w, b, cot = T.layer_case("train/dead", "3x3", 1, c_in, c_out, 2, 11, 37)
    conv = nn.Conv2d(c_in, c_out, 3, padding=1).cuda()
    bn = nn.BatchNorm2d(c_out, eps=R.NECK_EPS, momentum=0.01).cuda().train()
    with torch.no_grad():
        conv.weight.copy_(_dev(w))
        conv.bias.copy_(_dev(b))
        bn.bias[dead] = -60.0
    y = torch.relu(bn(rpn.conv2d_train(_dev(x), conv)))
    assert not bool(y[:, dead].any()) and bool(y[:, dead + 1].any())
    y.backward(_dev(cot))
    dw, db = conv.weight.grad.cpu().numpy(), conv.bias.grad.cpu().numpy()
    assert not dw[dead].any() and not np.signbit(dw[dead]).any() and db[dead] == 0 and not np.signbit(db[dead])
    assert dw[dead + 1].any() and np.isfinite(dw).all()


# ------------------------------------------------------------------------------------- the neck and the head
@functools.lru_cache(maxsize=None)
def _module_case(which, tag):
    """(x, cot, truth, f32) of the neck on canvas `tag`, or of the head on the neck's float64 train-mode output there"""
    B, _, H, W = R.CANVASES[tag]
    x = R.canvas(tag, R.CANVASES[tag])
    if which == "head":
        x = np.ascontiguousarray(_module_case("neck", tag)[2][0].astype(np.float32))
    module = (neck_module if which == "neck" else head_module)("cpu")
    cot = T.cotangent(f"{which}/{tag}", (B, 384 if which == "neck" else 11, H, W))
    truth, f32 = T.module_train(module, x, cot), T.module_train(module, x, cot, torch.float32)
    return x, cot, truth, f32


def _hold_module(row, m, out, dx, truth, f32, skip=()):
    _hold(f"{row}/out", out.detach().cpu().numpy(), f32[0], truth[0])
    if dx is not None:
        _hold(f"{row}/dx", dx.cpu().numpy(), f32[1], truth[1])
    params, zero = dict(m.named_parameters()), T.zero_by_batchnorm(m)
    assert set(params) == set(truth[2])
    for k in sorted(params):
        g = params[k].grad
        assert g is not None and bool(torch.isfinite(g).all()), k
        if k in zero:
            # the true gradient is zero: db = sum(dy) cancels to rounding. Held absolutely, against the same layer's dW: both are
            # sums of the same dy over the same pixels, dW's terms weighted by an input of order one
            assert float(g.abs().max()) <= 1e-4 * float(np.abs(truth[2][k.replace(".bias", ".weight")]).max()), k
        else:
            _hold(f"{row}/grad/{k}", g.cpu().numpy(), f32[2][k], truth[2][k], *T.grad_rows_kind(m, k))
    buffers = dict(m.named_buffers())
    assert set(buffers) == set(truth[3])
    for k in sorted(buffers):
        if k.endswith("num_batches_tracked"):
            assert int(buffers[k]) == int(truth[3][k]) == 8, k
        else:
            _hold(f"{row}/{k}", buffers[k].cpu().numpy(), f32[3][k], truth[3][k], "vector")


@pytest.mark.parametrize("tag", list(R.CANVASES))
@pytest.mark.parametrize("which", ["neck", "head"])
def test_train_forward_and_backward_against_float64(which, tag):
    x, cot, truth, f32 = _module_case(which, tag)
    m = (neck_module if which == "neck" else head_module)().train()
    xd, dcot = _dev(x).requires_grad_(), _dev(cot)
    warm = T.flat(m.train_forward(xd.detach()))             # the library is loaded and the allocator warm before the guard
    del warm
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in (R.neck_weights() if which == "neck" else R.head_weights()).items()})
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                 # nothing synchronises, in either direction
    try:
        out = T.flat(m.train_forward(xd))
        out.backward(dcot)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if which == "neck":
        got = out.detach().cpu().numpy()
        for c in (R.DEAD_CHANNEL, 128 + R.DEAD_CHANNEL, 256 + R.DEAD_CHANNEL):
            assert not truth[0][:, c].any() and not got[:, c].any()
    _hold_module(f"train/{which}/{tag}", m, out, xd.grad, truth, f32)
    # forward() in train mode is still the composite
    with torch.no_grad():
        again = T.flat(m(xd.detach()))
    assert again.shape == out.shape


@pytest.mark.parametrize("which", ["neck", "head"])
def test_train_forward_with_frozen_batchnorm_is_the_eval_forward(which):
    from rpn_gpu import dense_case
    x, n64, n32, h64, h32 = dense_case("a")
    m = (neck_module if which == "neck" else head_module)().train()
    for sub in m.modules():
        if isinstance(sub, nn.BatchNorm2d):
            sub.eval()
    inp = _dev(x if which == "neck" else n32).requires_grad_()
    out = T.flat(m.train_forward(inp))
    assert out.requires_grad
    truth, f32 = (n64, n32) if which == "neck" else (R.head_cat(R.head_f64(R.head_weights(), n32)), h32)
    _hold_forward(f"train/frozen/{which}", out.detach().cpu().numpy(), f32, truth)       # the forward's own bars
    with torch.no_grad():
        ev = T.flat(m.eval()(inp.detach()))
    _hold_forward(f"train/frozen/{which}/forward", ev.cpu().numpy(), f32, truth)
    assert all(int(v) == 7 for k, v in m.named_buffers() if k.endswith("num_batches_tracked"))
    out.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_train_forward_refuses_what_it_does_not_serve():
    neck = neck_module().train()
    with pytest.raises(RuntimeError, match="train_forward runs only on the GPU"):
        neck.train_forward(torch.zeros(R.CANVASES["a"]))
    with pytest.raises(ValueError, match="float32"):
        neck.train_forward(torch.zeros(R.CANVASES["a"], device="cuda", dtype=torch.float64))
    with pytest.raises(RuntimeError, match="DAL3_CONV2D_3X3 of stride 2"):     # the form without a dgrad kernel refuses by name
        hip.check(hip.lib().dal3_conv2d_dgrad_pack(hip.ptr(neck.blocks[0][1].weight), hip.CONV2D_1X1, 64, 64,
                                                   hip.ptr(neck.blocks[0][1].weight), None))


# ------------------------------------------------------------------------------------- the detector's first-stage loss
def test_first_stage_loss_on_the_hip_route():
    G = importlib.import_module("test_gpu_sparse_train")
    V = importlib.import_module("test_gpu_voxelnet")
    detector, pillars = V.detector, V.pillars
    center_loss = importlib.import_module("3dal_pytorch_amd.center_loss")
    pts, off = V.sweep()
    r = pillars.voxelize(G._dev(pts), off, V.VOXEL, V.RANGE, 5, 4000)
    voxels, coords, num, nv = r.finish()
    gt = np.zeros((2, 4, 10), np.float32)
    gt[0, 0] = [-1.5, 1.0, 0.0, 1.8, 4.2, 1.6, 0.3, 0, 0, 1]
    gt[0, 1] = [2.0, -2.5, 0.2, 0.7, 0.8, 1.7, -1.0, 0, 0, 2]
    gt[1, 0] = [0.5, 2.5, -0.1, 0.6, 1.7, 1.5, 2.0, 0, 0, 3]
    targets = center_loss.center_targets(G._dev(gt), [3], V.RANGE, V.VOXEL, 8, (2, 2))
    example = dict(voxels=voxels, coordinates=coords, num_points=num, num_voxels=nv, shape=[V.GRID] * 2, **targets)
    m = detector.VoxelNet(**V.MODEL, **V.KW)
    m.load_state_dict(V.checkpoint(), strict=True)
    m = m.cuda().train()
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    kept, inner_b, inner_h = {}, m.backbone.train_forward, m.bbox_head.train_forward

    def spy_backbone(*args, **kw):                          # keep the neck's input and d loss / d bev
        bev, levels = inner_b(*args, **kw)
        bev.retain_grad()
        kept["bev"] = bev
        return bev, levels

    def spy_head(x, **kw):                                  # keep the head's maps and d loss / d maps
        preds = inner_h(x, **kw)
        for d in preds:
            for v in d.values():
                v.retain_grad()
        kept["preds"] = preds
        return preds

    m.backbone.train_forward, m.bbox_head.train_forward = spy_backbone, spy_head
    with pytest.raises(ValueError, match="dense"):
        m.first_stage_loss(example, dense="stock")
    out = m.first_stage_loss(example, dense="hip")
    assert "preds" in kept, "dense='hip' did not run the head's train_forward"
    sum(out["loss"]).backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert float(sum(out["loss"]).detach()) > 0 and float(out["num_positive"][0]) > 0
    # the neck and the head under d loss / d maps as the cotangent, fed the same bev: float64 truth, fp32 CPU composite yardstick
    bev = kept["bev"].detach().cpu().numpy()
    cot = torch.cat([v.grad for d in kept["preds"] for v in d.values()], 1).cpu().numpy()
    assert np.abs(cot).max() > 0 and np.abs(bev).max() > 0
    fresh = detector.VoxelNet(**V.MODEL, **V.KW)
    fresh.load_state_dict(before, strict=True)
    truth = T.dense_train(fresh.neck, fresh.bbox_head, bev, cot)
    f32 = T.dense_train(fresh.neck, fresh.bbox_head, bev, cot, torch.float32)
    maps = torch.cat([v for d in kept["preds"] for v in d.values()], 1)
    _hold("first_stage/maps", maps.detach().cpu().numpy(), f32[0], truth[0])
    _hold("first_stage/dbev", kept["bev"].grad.cpu().numpy(), f32[1], truth[1])
    for i, (name, mod) in enumerate((("neck", m.neck), ("bbox_head", m.bbox_head))):
        params, zero = dict(mod.named_parameters()), T.zero_by_batchnorm(mod)
        for k in sorted(params):
            if k in zero:
                assert float(params[k].grad.abs().max()) <= 1e-4 * float(np.abs(truth[2][i][k.replace(".bias", ".weight")]).max()), k
            else:
                _hold(f"first_stage/{name}/grad/{k}", params[k].grad.cpu().numpy(), f32[2][i][k], truth[2][i][k], *T.grad_rows_kind(mod, k))
        for k, v in mod.named_buffers():
            if not k.endswith("num_batches_tracked"):
                _hold(f"first_stage/{name}/{k}", v.cpu().numpy(), f32[3][i][k], truth[3][i][k], "vector")
