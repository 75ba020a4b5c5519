"""The model of the dense stage's 16-bit arithmetic (tests/rpn_lp_model.py) judged on the CPU, and the `precision` plumbing
of rpn.RPN, rpn.CenterHead and the detector classes that needs no GPU.

The model's structure: with prec="fp32" (no rounding) it is the float64 chain of rpn_ref rounded to float32 after every
layer, and meets rpn_ref.BARS against the float64 truth with the torch-CPU composite as the yardstick. Its resolution: fp16
costs at least 10 x the fp32 yardstick's error, bf16 at least 4 x fp16 (three mantissa bits: 8 x expected). Planted
faults, each with the factor it must move the chain's rms error by:
  truncate            the mantissa cut instead of rounded to nearest even. A cut's relative error is one-sided on [0, u)
                      with rms u / sqrt(3), a rounding's is centred on [-u/2, u/2] with rms u / sqrt(12): twice the rms
                      per operand before the one-sided part, which does not cancel over a sum, adds to it. Bar: >= 2 x.
  weights_unrounded   the folded weights left float32. A product then carries one rounding instead of two independent
                      ones of the same size: sqrt(1/2) = 0.71 of the rms. Bar: within [0.6, 0.85] x."""
import importlib

import numpy as np
import pytest
import torch

import rpn_lp_model as M
import rpn_ref as R
from rpn_gpu import dense_case

rpn = importlib.import_module("3dal_pytorch_amd.rpn")
detector = importlib.import_module("3dal_pytorch_amd.detector")
two_stage = importlib.import_module("3dal_pytorch_amd.two_stage")
CANVASES = ("a", "b", "big")


def _hold(row, got, f32, truth):
    ratio, m, y = R.ratios(got, f32, truth)
    for k in R.MEASURES:
        print(f"{row:24s} {k:9s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:7.2f}  bar {R.BARS[k]:g}")
    assert m["dead_ok"]
    assert not [(k, ratio[k]) for k in R.MEASURES if ratio[k] > R.BARS[k]], row


_MODEL = {}


def model_case(tag, prec, fault=None):
    """(neck, head maps side by side) of the model on canvas `tag`, computed once"""
    key = (tag, prec, fault)
    if key not in _MODEL:
        x = dense_case(tag)[0]
        n = M.neck(R.neck_weights(), x, prec, fault)
        _MODEL[key] = (n, R.head_cat(M.head(R.head_weights(), n, prec, fault)))
    return _MODEL[key]


@pytest.mark.parametrize("tag", CANVASES)
def test_without_rounding_the_model_is_the_float64_chain(tag):
    x, n64, n32, h64, h32 = dense_case(tag)
    n, h = model_case(tag, "fp32")
    assert n.dtype == h.dtype == np.float32 and n.shape == n64.shape and h.shape == h64.shape
    _hold(f"model/fp32/neck/{tag}", n, n32, n64)
    _hold(f"model/fp32/head/{tag}", h, h32, h64)


def test_the_f64_mode_is_the_float64_truth_for_any_configuration():
    x, n64, _, h64, _ = dense_case("a")
    n = M.neck(R.neck_weights(), x, "f64")
    assert n.dtype == np.float64 and np.array_equal(n, n64)
    assert np.array_equal(R.head_cat(M.head(R.head_weights(), n, "f64")), h64)
    # another neck: two blocks, the first without a deblock; its chain is the production one's first layers
    sd = R.neck_weights()
    small = dict(layer_nums=[3, 5], ds_layer_strides=[1, 2], us_layer_strides=[2])
    sd2 = {k: v for k, v in sd.items() if k.startswith(("blocks.0.", "blocks.1."))}
    sd2.update({k.replace("deblocks.1.", "deblocks.0."): v for k, v in sd.items() if k.startswith("deblocks.1.")})
    assert np.array_equal(M.neck(sd2, x, "f64", cfg=small), n64[:, 128:256])
    assert np.array_equal(M.neck(sd2, x, "fp16", cfg=small), model_case("a", "fp16")[0][:, 128:256])


@pytest.mark.parametrize("tag", CANVASES)
def test_the_model_has_resolution(tag):
    x, n64, n32, h64, h32 = dense_case(tag)
    for what, truth, f32, at in (("neck", n64, n32, 0), ("head", h64, h32, 1)):
        yard = M.errors(f32, truth)
        e16, eb16 = M.errors(model_case(tag, "fp16")[at], truth), M.errors(model_case(tag, "bf16")[at], truth)
        for k in ("rms", "max"):
            print(f"{what}/{tag} {k}: yardstick {yard[k]:.3e}  fp16 {e16[k]:.3e}  bf16 {eb16[k]:.3e}")
        assert e16["rms"] >= 10 * yard["rms"] and eb16["rms"] >= 4 * e16["rms"], (what, tag)
        # the model stays where the issue's table puts it: within a factor 2 of its ends
        lo, hi = {"neck": ((1.0e-3, 2.2e-3), (7.9e-3, 1.8e-2)), "head": ((1.6e-3, 3.4e-3), (1.2e-2, 2.7e-2))}[what]
        assert lo[0] / 2 <= e16["rms"] <= lo[1] * 2 and hi[0] / 2 <= eb16["rms"] <= hi[1] * 2, (what, tag)


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_planted_faults_move_the_chain(prec):
    x, n64, n32, h64, h32 = dense_case("a")
    for what, truth, at in (("neck", n64, 0), ("head", h64, 1)):
        base = M.errors(model_case("a", prec)[at], truth)["rms"]
        cut = M.errors(model_case("a", prec, "truncate")[at], truth)["rms"]
        raw = M.errors(model_case("a", prec, "weights_unrounded")[at], truth)["rms"]
        print(f"{what}/{prec}: model {base:.3e}  truncate x {cut / base:.2f}  weights_unrounded x {raw / base:.2f}")
        assert cut >= 2.0 * base, (what, "truncate", cut / base)
        assert 0.6 * base <= raw <= 0.85 * base, (what, "weights_unrounded", raw / base)


def test_q_rounds_to_nearest_even():
    ties = np.asarray([1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11], np.float32)
    assert M.q(ties, "fp16").tolist() == [1 + 2.0 ** -10, 1.0, 1 + 2.0 ** -9]
    ties = np.asarray([1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], np.float32)
    assert M.q(ties, "bf16").tolist() == [1 + 2.0 ** -7, 1.0, 1 + 2.0 ** -6]
    assert M.q(ties, "fp32") is not None and np.array_equal(M.q(ties, "fp32"), ties)
    assert M._truncated(ties, "bf16").tolist() == [1.0, 1.0, 1 + 2.0 ** -7]
    assert np.isinf(M.q(np.asarray([65520.0], np.float32), "fp16")).all() and M.q(np.asarray([65519.0], np.float32), "fp16")[0] == 65504.0


# ------------------------------------------------------------------------------------- the plumbing
PP_MODEL = dict(reader=dict(type="PillarFeatureNet", num_filters=[64, 64], num_input_features=5, with_distance=False,
                            voxel_size=(0.32, 0.32, 6.0), pc_range=(0.0, -5.76, -2.0, 14.08, 5.76, 4.0)),
                backbone=dict(type="PointPillarsScatter", ds_factor=1), neck=dict(type="RPN", **R.NECK),
                bbox_head=dict(type="CenterHead", **R.HEAD))
VN_MODEL = dict(reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5),
                backbone=dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8),
                neck=dict(type="RPN", layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[32, 64], us_layer_strides=[1, 2],
                          us_num_filters=[64, 64], num_input_features=256),
                bbox_head=dict(type="CenterHead", **dict(R.HEAD, in_channels=128)))


def test_precision_is_validated_everywhere():
    import roi_ref
    neck, head = rpn.RPN(**R.NECK), rpn.CenterHead(**R.HEAD)
    pp, vn = detector.PointPillars(**PP_MODEL), detector.VoxelNet(**VN_MODEL)
    ts = two_stage.TwoStageDetector(dict(type="PointPillars", **PP_MODEL),
                                    [dict(type="BEVFeatureExtractor", pc_start=[0.0, -5.76], voxel_size=[0.32, 0.32], out_stride=1)],
                                    dict(type="RoIHead", input_channels=384, model_cfg=roi_ref.PRODUCTION, code_size=7), 100)
    for m in (neck, head, pp, vn, ts):
        assert m.precision == "fp32"
        for bad, why in (("f16x3", "point heads only"), ("fp64", "unknown precision"), (None, "unknown precision"), ("FP16", "unknown")):
            with pytest.raises(ValueError, match=why):
                m.precision = bad
            assert m.precision == "fp32"
        for ok in ("fp16", "bf16", "fp32"):
            m.precision = ok
            assert m.precision == ok
    pp.precision = "bf16"
    assert pp.neck.precision == pp.bbox_head.precision == "bf16"
    ts.precision = "fp16"
    assert ts.single_det.precision == ts.single_det.neck.precision == ts.bbox_head.precision == "fp16"
    assert not hasattr(ts.roi_head, "precision") and not hasattr(ts.single_det.reader, "precision")
    for bad in ("f16x3", "int8"):
        with pytest.raises(ValueError):
            rpn.check_precision(bad)
        with pytest.raises(ValueError):
            rpn.pack_layer(neck.blocks[0][1], neck.blocks[0][2], 0, precision=bad)
        with pytest.raises(ValueError):
            rpn.conv2d(torch.zeros(1, 64, 4, 4), torch.zeros(4), 0, 1, True, 64, precision=bad)
    assert [rpn.check_precision(p) for p in rpn.PRECISIONS] == [0, 2, 1]


def test_train_mode_ignores_precision():
    neck, head = rpn.RPN(**R.NECK), rpn.CenterHead(**R.HEAD)
    x = torch.from_numpy(R.canvas("a", R.CANVASES["a"]))
    with torch.no_grad():
        want_n = neck.train()(x)
        want_h = head.train()(want_n)
    neck.precision = head.precision = "fp16"
    with torch.no_grad():
        got_n = neck(x)
        got_h = head(got_n)
    # (train-mode BatchNorm normalises by the batch's own statistics: the same composite twice gives the same bits)
    assert got_n.dtype == torch.float32 and torch.equal(got_n, want_n)
    assert all(torch.equal(got_h[0][k], want_h[0][k]) for k in want_h[0])
    neck.eval(), head.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        neck(x)                                      # eval mode is the kernel route, in every precision


def test_the_cache_key_changes_with_precision(monkeypatch):
    calls = []

    def fake_pack(conv, bn, kind, precision="fp32", name=None, check=True):
        calls.append((name, precision))
        return torch.zeros(8 + 4 * 4 * conv.out_channels, dtype=torch.float32 if precision == "fp32" else torch.uint8)

    checked = []
    monkeypatch.setattr(rpn, "pack_layer", fake_pack)
    monkeypatch.setattr(rpn, "refuse_nonfinite_weights", lambda packs, layers, precision: checked.append((len(packs), precision)))
    neck, head = rpn.RPN(**R.NECK).eval(), rpn.CenterHead(**R.HEAD).eval()
    for m, n_layers, first in ((neck, 19, "blocks.0.1"), (head, 11, "shared_conv.0")):
        calls.clear()
        a = m.packed()
        assert m.packed() is a and len(calls) == n_layers and calls[0] == (first, "fp32")
        m.precision = "fp16"
        b = m.packed()
        assert b is not a and m.packed() is b and len(calls) == 2 * n_layers and calls[-1][1] == "fp16"
        m.precision = "fp16"                                         # the same value: no repack
        assert m.packed() is b
        m.precision = "fp32"
        c = m.packed()
        assert c is not b and len(calls) == 3 * n_layers and calls[-1][1] == "fp32"
    # one range check per 16-bit packing, over all of a module's blobs; none for fp32
    assert checked == [(19, "fp16"), (11, "fp16")]
    # the head's fused first layers are built in every precision: biases first (4 bytes a row in a 16-bit blob)
    packs, fused = head.packed()
    assert fused[0] is not None and fused[0].dtype == torch.float32 and fused[0].numel() == 5 * packs[1].numel()
    head.precision = "bf16"
    packs, fused = head.packed()
    assert fused[0].dtype == torch.uint8 and fused[0].numel() == 5 * packs[1].numel()


def test_lp_flop_counts_sixteen_channel_steps():
    assert rpn.conv2d_lp_flop(0, 1, 24, 40, 11, 37) == (2 * 11 * 37 * 40 * 24 * 9, 2 * 16 * 64 * 64 * 32 * 9)
    assert rpn.conv2d_flop(0, 1, 24, 40, 11, 37)[1] == 2 * 16 * 64 * 64 * 24 * 9
