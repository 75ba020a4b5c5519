"""CPU-side checks of the dense stage's training route (tests/rpn_train_ref.py; 3dal_pytorch_amd/rpn.py, detector.py): the
written-out backward sums against stock autograd in float64 on every form, the planted faults against the GPU tests' bars,
the refusals of `train_forward` and the `dense=` keyword, and the new entries' argument checks. These validate the
yardstick; no GPU compute here."""
import importlib
import inspect

import numpy as np
import pytest
import torch
from torch import nn

import rpn_ref as R
import rpn_train_ref as T

hip = importlib.import_module("3dal_pytorch_amd._hip")
rpn = importlib.import_module("3dal_pytorch_amd.rpn")
detector = importlib.import_module("3dal_pytorch_amd.detector")

# the smallest ratio a planted fault reached over the measures and the cases below (printed by
# test_planted_faults_exceed_ten_times_every_bar): every bar of rpn_train_ref.BARS stays under a tenth of it
SMALLEST_FAULT_RATIO = 1e5                      # recorded 1.89e5 (cat_slice_offset, deblocks.2.0.weight on canvas b, chan_max)
# H and W both even and odd: with H even a stride-2 layer never reads the bottom padding row, with H odd it does
SIZES = ((6, 8), (7, 9), (6, 9), (11, 37))


@pytest.fixture(autouse=True)
def _grad_on():
    """whatever a test before this file left switched"""
    with torch.enable_grad():
        yield


def _close(a, b, what):
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), what


@pytest.mark.parametrize("kind,stride", T.FORMS)
@pytest.mark.parametrize("c", [1, 3, 24, 40])
def test_written_out_sums_equal_autograd(kind, stride, c):
    for H, W in SIZES[:3] if c != 24 else SIZES:
        for c_in, c_out in ((c, 5), (7, c)):
            x, w, b, cot = T.layer_case(f"sums/{kind}{stride}/{c_in}-{c_out}/{H}x{W}", kind, stride, c_in, c_out, 2, H, W)
            y, dx, dw, db = T.layer_autograd(x, w, b, kind, stride, cot)
            assert y.shape[2:] == T.out_size(kind, stride, H, W) == cot.shape[2:]
            _close(T.dgrad_sum(cot, w, kind, stride, H, W), dx, "dx")
            _close(T.wgrad_sum(x, cot, kind, stride), dw, "dW")
            _close(T.db_sum(cot), db, "db")
            _close(R.form(x, w, kind, stride) + b.astype(np.float64).reshape(1, -1, 1, 1), y, "y")


def _layer_fault_rows():
    """(fault, row name, faulty, yardstick, truth, what, kind) for every layer-level fault on every form it acts on"""
    for kind, stride in T.FORMS:
        for H, W in ((12, 12), (13, 37)):
            tag = f"fault/{kind}{stride}/{H}x{W}"
            x, w, b, cot = T.layer_case(tag, kind, stride, 24, 40, 2, H, W)
            _, dx, dw, db = T.layer_autograd(x, w, b, kind, stride, cot)
            _, dx32, dw32, db32 = T.layer_autograd(x, w, b, kind, stride, cot, torch.float32)
            k = "deconv" if kind == "deconv" else None
            if kind == "3x3":
                yield "dgrad_taps_not_flipped", tag, T.dgrad_sum(cot, w, kind, stride, H, W, "dgrad_taps_not_flipped"), dx32, dx, "map", k
                yield "wgrad_across_border", tag, T.wgrad_sum(x, cot, kind, stride, "wgrad_across_border"), dw32, dw, "weight", k
            if kind == "3x3" and stride == 2:
                yield "stride2_phase_shifted", tag, T.dgrad_sum(cot, w, kind, stride, H, W, "stride2_phase_shifted"), dx32, dx, "map", k
            if kind == "deconv":
                yield "deconv_dydx_swapped", tag + "/dx", T.dgrad_sum(cot, w, kind, stride, H, W, "deconv_dydx_swapped"), dx32, dx, "map", k
                yield "deconv_dydx_swapped", tag + "/dW", T.wgrad_sum(x, cot, kind, stride, "deconv_dydx_swapped"), dw32, dw, "weight", k
            yield "bias_grad_dropped", tag, T.db_sum(cot, "bias_grad_dropped"), db32, db, "vector", k


def _neck(weights=True):
    m = rpn.RPN(**R.NECK)
    if weights:
        m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in R.neck_weights().items()}, strict=True)
    return m


def _head():
    m = rpn.CenterHead(**R.HEAD)
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in R.head_weights().items()}, strict=True)
    return m


def test_planted_faults_exceed_ten_times_every_bar():
    smallest, seen = np.inf, set()
    for fault, row, bad, f32, truth, what, kind in _layer_fault_rows():
        ratio = T.ratios(bad, f32, truth, what, kind)[0]
        seen.add(fault)
        for k in T.MEASURES:
            print(f"{fault:24s} {row:28s} {k:9s} ratio {ratio[k]:12.4g}")
            assert ratio[k] >= 10 * T.BARS[k], (fault, row, k, ratio[k])
            smallest = min(smallest, ratio[k])
    # a cat slice offset by one deblock: the neck's gradients under a cotangent read one slice along
    neck = _neck()
    for tag, shape in R.CANVASES.items():
        x = R.canvas(tag, shape)
        cot = T.cotangent(f"neck/{tag}", (shape[0], 384, shape[2], shape[3]))
        _, dx, grads, _ = T.module_train(neck, x, cot)
        _, dx32, grads32, _ = T.module_train(neck, x, cot, torch.float32)
        _, bdx, bgrads, _ = T.module_train(neck, x, cot, fault="cat_slice_offset")
        rows = [("dx", bdx, dx32, dx, "map", None)]
        rows += [(k, bgrads[k], grads32[k], grads[k], *T.grad_rows_kind(neck, k)) for k in ("deblocks.0.0.weight", "deblocks.2.0.weight",
                                                                                          "blocks.0.1.weight")]
        for name, bad, f32, truth, what, kind in rows:
            ratio = T.ratios(bad, f32, truth, what, kind)[0]
            for k in T.MEASURES:
                print(f"{'cat_slice_offset':24s} {tag + '/' + name:28s} {k:9s} ratio {ratio[k]:12.4g}")
                assert ratio[k] >= 10 * T.BARS[k], (tag, name, k, ratio[k])
                smallest = min(smallest, ratio[k])
    seen.add("cat_slice_offset")
    assert seen == set(T.FAULTS)
    print(f"smallest planted-fault ratio {smallest:.3g}")
    assert smallest >= SMALLEST_FAULT_RATIO and all(b <= SMALLEST_FAULT_RATIO / 10 for b in T.BARS.values())


def test_module_truth_is_autograd_through_the_written_out_layers():
    """one deblock of the neck by hand: the module-level truth and the layer-level sums describe the same backward"""
    neck = _neck().double().train()
    x = torch.tensor(R.canvas("a", R.CANVASES["a"]), dtype=torch.float64)
    with torch.no_grad():
        mid = neck.blocks[1](neck.blocks[0](x))
    conv = neck.deblocks[1][0]
    mid = mid.clone().requires_grad_()
    y = conv(mid)
    cot = torch.tensor(T.cotangent("deblock1", tuple(y.shape)), dtype=torch.float64)
    y.backward(cot)
    w = conv.weight.detach().numpy()
    _close(T.dgrad_sum(cot.numpy(), w, "deconv", 2, *mid.shape[2:]), mid.grad.numpy(), "dx")
    _close(T.wgrad_sum(mid.detach().numpy(), cot.numpy(), "deconv", 2), conv.weight.grad.numpy(), "dW")


def test_zero_by_batchnorm_names_the_heads_biases():
    head = _head()
    names = T.zero_by_batchnorm(head)
    assert names == {"shared_conv.0.bias"} | {f"tasks.0.{h}.0.bias" for h in R.HEAD_ORDER}
    x = R.canvas("a", (2, 384, 8, 12))
    _, _, grads, stats = T.module_train(head, x, T.cotangent("head/zero", (2, 11, 8, 12)))
    for k in names:
        assert np.abs(grads[k]).max() <= 1e-12 * np.abs(grads[k.replace(".bias", ".weight")]).max(), k
    assert int(stats["shared_conv.1.num_batches_tracked"]) == 8 and T.zero_by_batchnorm(_neck()) == set()


def test_train_forward_refuses_in_words():
    neck, head = _neck(), _head()
    x = torch.zeros(R.CANVASES["a"])
    for m, inp in ((neck, x), (head, torch.zeros((1, 384, 4, 4)))):
        with pytest.raises(RuntimeError, match="train_forward runs only on the GPU"):
            m.train_forward(inp)
    gn = rpn.RPN(**dict(R.NECK, norm_cfg=dict(type="GN", num_groups=8)))
    assert not gn.hip_serves()
    with pytest.raises(NotImplementedError, match="GroupNorm.* is not an affine nn.BatchNorm2d with running statistics"):
        gn.train_forward(x)
    plain = _neck()
    plain.blocks[0][2] = nn.BatchNorm2d(64, affine=False)
    with pytest.raises(NotImplementedError, match="is not an affine nn.BatchNorm2d with running statistics"):
        plain.train_forward(x)
    strided = rpn.RPN(**dict(R.NECK, us_layer_strides=[0.5, 1, 2]))
    assert not strided.hip_serves()
    with pytest.raises(NotImplementedError, match="does not serve"):
        strided.train_forward(x)
    # forward() in train mode keeps returning the composite
    neck.train()
    with torch.no_grad():
        assert torch.equal(neck(x), neck.composite(x))


def test_dense_keyword_defaults_to_composite_and_refuses_other_words():
    for fn in (detector.VoxelNet.first_stage_loss, detector.VoxelNet.train_step_from_sweeps):
        assert inspect.signature(fn).parameters["dense"].default == "composite"
    assert detector.DENSE_ROUTES == ("composite", "hip")
    m = detector.VoxelNet.__new__(detector.VoxelNet)
    with pytest.raises(ValueError, match="'composite' \\(stock torch\\) or 'hip'"):
        detector.VoxelNet.first_stage_loss(m, {}, dense="triton")


def test_entries_refuse_bad_arguments_and_state_the_workspace():
    lib = hip.lib()
    K = hip
    assert hip.CONV2D_WGRAD_SLICE == 4096
    # the workspace formula of the header
    for kind, s, c_in, c_out, B, H, W in ((K.CONV2D_3X3, 1, 256, 256, 4, 188, 188), (K.CONV2D_3X3, 2, 128, 256, 1, 188, 188),
                                          (K.CONV2D_1X1, 1, 64, 3, 2, 5, 7), (K.CONV2D_DECONV2, 2, 128, 128, 1, 94, 94),
                                          (K.CONV2D_DECONV4, 4, 256, 128, 1, 47, 47)):
        tc = 16 if kind == K.CONV2D_DECONV4 else 32
        ph, pw = ((H - 1) // s + 1, (W - 1) // s + 1) if kind == K.CONV2D_3X3 else (H, W)
        taps = 9 if kind == K.CONV2D_3X3 else 1 if kind == K.CONV2D_1X1 else s * s
        tiles = B * -(-ph // 4) * -(-pw // tc)
        want = 4 * c_in * c_out * taps * -(-tiles // (hip.CONV2D_WGRAD_SLICE // (4 * tc)))
        assert lib.dal3_conv2d_wgrad_workspace_bytes(kind, s, c_in, c_out, B, H, W) == want
    assert lib.dal3_conv2d_wgrad_workspace_bytes(K.CONV2D_3X3, 1, 256, 256, 4, 188, 188) == 36 * 4 * 256 * 256 * 9
    assert lib.dal3_conv2d_wgrad_workspace_bytes(K.CONV2D_3X3, 3, 8, 8, 1, 8, 8) == 0
    assert lib.dal3_conv2d_wgrad_workspace_bytes(K.CONV2D_1X1, 1, 8, 5000, 1, 8, 8) == 0
    assert lib.dal3_conv2d_dgrad_pack_floats(K.CONV2D_1X1, 8, 8) == 0
    assert lib.dal3_conv2d_dgrad_pack_floats(K.CONV2D_3X3, 24, 40) == 1 * 5 * 9 * 256
    assert lib.dal3_conv2d_dgrad_pack_floats(K.CONV2D_DECONV4, 40, 3) == 2 * 6 * 256
    one = hip.Map(1, 1, 1, 1, 1)                    # never dereferenced: every call below is refused before a launch
    good = dict(kind=K.CONV2D_3X3, stride=2, c_in=8, c_out=8, B=1, H=4, W=4, dy=one, dx=one, packed=16)
    for change in (dict(kind=K.CONV2D_1X1), dict(stride=1), dict(c_in=0), dict(c_out=4097), dict(H=65536), dict(B=-1),
                   dict(max_workgroups=-1), dict(reserved=1), dict(packed=8), dict(packed=None), dict(dx=hip.Map(None, 1, 1, 1, 1)),
                   dict(kind=K.CONV2D_DECONV4, stride=2), dict(kind=K.CONV2D_DECONV4, stride=4, H=20000)):
        assert lib.dal3_conv2d_dgrad(hip.Conv2dDgradArgs(**dict(good, **change)), None) == hip.EINVAL, change
    good = dict(kind=K.CONV2D_3X3, stride=1, c_in=8, c_out=8, B=1, H=4, W=4, x=one, dy=one, dw=16, db=None, workspace=16,
                workspace_bytes=1 << 20)
    for change in (dict(kind=4), dict(stride=3), dict(kind=K.CONV2D_1X1, stride=2), dict(c_in=0), dict(W=-1), dict(dw=None),
                   dict(max_workgroups=-1), dict(reserved=2), dict(workspace=None), dict(workspace=12), dict(x=hip.Map(None, 1, 1, 1, 1))):
        assert lib.dal3_conv2d_wgrad(hip.Conv2dWgradArgs(**dict(good, **change)), None) == hip.EINVAL, change
    assert lib.dal3_conv2d_wgrad(hip.Conv2dWgradArgs(**dict(good, workspace_bytes=8)), None) == hip.EWORKSPACE
    assert lib.dal3_conv2d_dgrad_pack(None, K.CONV2D_3X3, 8, 8, 16, None) == hip.EINVAL
    assert lib.dal3_conv2d_dgrad_pack(16, K.CONV2D_1X1, 8, 8, 16, None) == hip.EINVAL
    assert lib.dal3_conv2d_dgrad_pack(16, K.CONV2D_3X3, 8, 8, 24, None) == hip.EINVAL
