"""The detector's 2-D convolutions on the GPU (3dal_pytorch_amd/rpn.py; dal3_conv2d_pack / dal3_conv2d): impulses pin
the tap orientation, the padding, the stride-2 phase, the transposed convolutions' sub-positions and the channel slice
bit for bit; single layers and the whole neck and head are judged against the float64 restatement of tests/rpn_ref.py
with the torch-CPU fp32 layer / module as the yardstick, under rpn_ref.BARS. The shapes are the smallest that cross each
seam of the kernel: its 8 x 32 pixel tile, its 32-row channel tile, its 16- (stride 1) and 8-channel (stride 2) chunks.

With DAL3_RPN_RECORD=<path> in the environment the run also writes every measure, yardstick and ratio to <path>
(tests/rpn_gpu.py; how profiles/rpn_measured.json was made)."""
import numpy as np
import pytest
import torch

import rpn_ref as R
from rpn_gpu import (_dev, _hold, _record_file, dense_case, head_module, layer_params, neck_module, rpn, run_layer,  # noqa: F401
                     yardstick)

pytestmark = pytest.mark.gpu

FORMS = (("3x3", 1), ("3x3", 2), ("1x1", 1), ("deconv", 2), ("deconv", 4))
IMPULSE = dict(B=2, c_in=24, c_out=40, H=11, W=37, offset=3, channels=50)      # two tiles each way; 24 = a chunk and a half
SENTINEL = -7.5


def _impulse_expected(wf, bf, kind, s, b0, c0, y0, x0, relu):
    """relu(fl32(W'[tap] + b')) where the impulse reaches, relu(b') elsewhere -> (B, c_out, OH, OW) float32"""
    I = IMPULSE
    OH, OW = ((I["H"] - 1) // s + 1, (I["W"] - 1) // s + 1) if kind == "3x3" else (I["H"] * s, I["W"] * s) if kind == "deconv" \
        else (I["H"], I["W"])
    out = np.broadcast_to(bf.reshape(1, -1, 1, 1), (I["B"], I["c_out"], OH, OW)).copy()
    if kind == "3x3":
        for ky in range(3):
            for kx in range(3):
                ny, nx = y0 + 1 - ky, x0 + 1 - kx               # oy * s + ky - 1 = y0
                if ny % s == 0 and nx % s == 0 and 0 <= ny // s < OH and 0 <= nx // s < OW:
                    out[b0, :, ny // s, nx // s] = wf[:, c0, ky, kx] + bf
    elif kind == "1x1":
        out[b0, :, y0, x0] = wf[:, c0, 0, 0] + bf
    else:
        for dy in range(s):
            for dx in range(s):
                out[b0, :, y0 * s + dy, x0 * s + dx] = wf[c0, :, dy, dx] + bf
    assert out.dtype == np.float32
    return np.maximum(out, np.float32(0)) if relu else out


@pytest.mark.parametrize("kind,stride", FORMS)
def test_impulses_are_bit_exact(kind, stride):
    I = IMPULSE
    w, b, bn = layer_params(f"impulse/{kind}{stride}", kind, stride, I["c_in"], I["c_out"], True, True)
    wf, bf = R.fold(w, b, bn, R.NECK_EPS, deconv=kind == "deconv")
    assert (bf < 0).any() and (bf > 0).any()
    H, W = I["H"], I["W"]
    spots = [(y, x) for y in (0, H // 2, H - 1) for x in (0, W // 2, W - 1)]       # corners, edges, the interior
    spots += [(7, 31), (8, 32)]                                                      # either side of the tile seams
    x = torch.zeros((I["B"], I["c_in"], H, W), device="cuda")
    n = 0
    for b0 in range(I["B"]):
        for c0 in (0, I["c_in"] - 1):
            for y0, x0 in spots:
                x.zero_()
                x[b0, c0, y0, x0] = 1.0
                want = _impulse_expected(wf, bf, kind, stride, b0, c0, y0, x0, True)
                out = torch.full((I["B"], I["channels"]) + want.shape[2:], SENTINEL, device="cuda")
                y = run_layer(x, w, b, bn, R.NECK_EPS, kind, stride, True, out=out, channel_offset=I["offset"])
                got = out.cpu().numpy()
                assert y.data_ptr() == out[:, I["offset"]:].data_ptr()
                assert np.array_equal(got[:, I["offset"]:I["offset"] + I["c_out"]].view(np.uint32), want.view(np.uint32)), (b0, c0, y0, x0)
                rest = np.delete(got, np.s_[I["offset"]:I["offset"] + I["c_out"]], axis=1)
                assert (rest == SENTINEL).all(), "a channel outside the slice was written"
                n += 1
    assert n == 2 * 2 * 11
    # without ReLU the negative values come through
    want = _impulse_expected(wf, bf, kind, stride, 1, 0, H - 1, W - 1, False)
    x.zero_()
    x[1, 0, H - 1, W - 1] = 1.0
    got = run_layer(x, w, b, bn, R.NECK_EPS, kind, stride, False).cpu().numpy()
    assert (want < 0).any() and np.array_equal(got.view(np.uint32), want.view(np.uint32))


PAIRS = ((64, 64), (64, 128), (128, 256), (256, 256), (384, 64), (64, 1), (64, 2), (64, 3))
# (canvas, B, kind, stride, relu, bias, bn, input view, max_workgroups): every canvas, form, stride, option and view at
# least once per channel pair
SCHEDULE = (((5, 7), 2, "3x3", 1, True, False, True, "plain", 0),
            ((12, 12), 1, "3x3", 2, False, True, False, "sliced", 1),
            ((13, 37), 2, "3x3", 2, True, True, True, "channels_last", 3),
            ((36, 44), 1, "3x3", 1, True, True, True, "plain", 0),
            ((13, 37), 1, "1x1", 1, True, False, True, "sliced", 3),
            ((5, 7), 2, "deconv", 2, True, False, True, "channels_last", 1),
            ((12, 12), 1, "deconv", 4, False, True, True, "plain", 0))


def _view(x, how):
    """the same values behind other strides: a slice of a larger tensor, or channels-last memory"""
    t = _dev(x)
    if how == "sliced":
        big = torch.full((t.shape[0], 2 * t.shape[1], t.shape[2] + 3, t.shape[3] + 5), float("nan"), device="cuda")
        big[:, ::2, 1:-2, 2:-3] = t
        t = big[:, ::2, 1:-2, 2:-3]
    elif how == "channels_last":
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert t.shape == x.shape and (how == "plain") == t.is_contiguous()
    return t


@pytest.mark.parametrize("case", range(len(SCHEDULE)))
@pytest.mark.parametrize("c_in,c_out", PAIRS)
def test_single_layers_against_float64(c_in, c_out, case):
    (H, W), B, kind, stride, relu, bias, bn_on, how, wg = SCHEDULE[case]
    tag = f"layer/{c_in}-{c_out}/{kind}{stride}/{H}x{W}"
    w, b, bn = layer_params(tag, kind, stride, c_in, c_out, bias, bn_on)
    x = R.synth.uniform(R.SEED, tag + "/x", (B, c_in, H, W), 0.0, 2.0).astype(np.float32)
    x *= R.synth.uniform(R.SEED, tag + "/live", (B, 1, H, W)) < 0.6
    eps = R.NECK_EPS if kind != "3x3" or stride == 2 else R.HEAD_EPS
    truth = R.layer(x, w, b, bn, eps, kind, stride, relu)
    if kind == "3x3" and stride == 2:
        assert truth.shape[2:] == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    f32 = yardstick(x, w, b, bn, eps, kind, stride, relu)
    got = run_layer(_view(x, how), w, b, bn, eps, kind, stride, relu, max_workgroups=wg).cpu().numpy()
    assert got.shape == truth.shape == f32.shape
    _hold(tag + f"/wg{wg}", got, f32, truth)


@pytest.mark.parametrize("tag", ["a", "b", "big"])
def test_whole_neck_and_head_against_float64(tag):
    x, n64, n32, h64, h32 = dense_case(tag)
    neck, head = neck_module(), head_module()
    assert neck.hip_serves() and head.hip_serves()
    with torch.no_grad():
        n = neck(_dev(x))
        preds = head(n)
    assert n.shape == n64.shape and n.is_contiguous()
    got_n = n.cpu().numpy()
    for c in (R.DEAD_CHANNEL, 128 + R.DEAD_CHANNEL, 256 + R.DEAD_CHANNEL):
        assert not n64[:, c].any() and not got_n[:, c].any() and not np.signbit(got_n[:, c]).any()
    _hold(f"neck/{tag}", got_n, n32, n64)
    assert list(preds[0]) == list(R.HEAD_ORDER) and [preds[0][k].shape[1] for k in R.HEAD_ORDER] == [2, 1, 3, 2, 3]
    _hold(f"head/{tag}", R.head_cat([{k: v.cpu().numpy() for k, v in d.items()} for d in preds]), h32, h64)
    # the head alone, on the yardstick's own input
    alone = head(_dev(n32))
    with torch.no_grad():
        h64_alone = R.head_cat(R.head_f64(R.head_weights(), n32))
    _hold(f"head_alone/{tag}", R.head_cat([{k: v.cpu().numpy() for k, v in d.items()} for d in alone]), h32, h64_alone)


def test_results_do_not_depend_on_the_grid_and_the_cache_follows_the_weights():
    x, n64, n32, _, _ = dense_case("a")
    neck = neck_module()
    with torch.no_grad():
        a = neck(_dev(x)).cpu().numpy()
        b = neck(_dev(x), max_workgroups=3).cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        packed = neck.packed()
        assert neck.packed() is packed
        neck.blocks[0][1].weight.mul_(2.0)                      # a version bump: the cache is rebuilt
        assert neck.packed() is not packed
        c = neck(_dev(x)).cpu().numpy()
        assert not np.array_equal(a, c)
        neck.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in R.neck_weights().items()})
        assert np.array_equal(neck(_dev(x)).cpu().numpy().view(np.uint32), a.view(np.uint32))
    # train mode is the composite, on any device
    assert neck.train().composite(_dev(x)).shape == a.shape
