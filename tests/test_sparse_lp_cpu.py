"""The model of the sparse middle's 16-bit arithmetic (tests/sparse_lp_model.py) judged on the CPU, and the
`sparse_precision` plumbing of sparse.py and the detector classes that needs no GPU.

The model's structure: with prec="f64" it IS sparse_ref.backbone. Its resolution: fp16 costs at least 100 x the fp32
yardstick's error (13 mantissa bits apart: 8192 x per rounding), bf16 about 8 x fp16 (three mantissa bits; held to 4 .. 16).
Planted faults, each with what it must move the chain's rms error against the float64 truth by:
  truncate            the mantissa cut instead of rounded to nearest even: a cut's relative error is one-sided on [0, u)
                      with rms u / sqrt(3), a rounding's is centred with rms u / sqrt(12): twice the rms per operand before
                      the one-sided part, which does not cancel over a sum, adds to it. Bar: >= 2 x.
  weights_unrounded   the folded weights left float32: a product carries one rounding instead of two independent ones of
  inputs_unrounded    the same size, and so it does with the gathered activations left float32: sqrt(1/2) = 0.71 of the
                      rms. Bar: within [0.6, 0.85] x, which is below 1 / emu16.RMS_SLACK = 0.87.
  residual_rounded    the block input rounded before it is added. It is one more rounding of ONE activation-sized term next
                      to the roundings of a sum's 27 c products, so the chain's error against the truth hardly grows
                      (measured 0.99 .. 1.12 x); what it moves is the RESULT: the distance between the faulty chain and
                      the model, in units of the model's own error. A block's output carries the residual's rounding at
                      full size (rms u / sqrt(12) of the residual), the same size as the rounding of the next layer's
                      input that the model's error is made of. Bar: that rms distance >= emu16.RMS_SLACK - 1 = 0.15 of
                      the model's rms error, on every level. (The largest difference is printed, not held: it is one
                      element, and nothing ties it to the element where the model's own error peaks.)
Every fault's rms distance from the model is held to that bar: a kernel that computes a faulty chain is further from the
model than the rms slack of tests/test_gpu_sparse_lp.py's chain bar."""
import importlib

import numpy as np
import pytest
import torch

import sparse_lp_model as L
import sparse_ref as S
from emu16 import RMS_SLACK

hip = importlib.import_module("3dal_pytorch_amd._hip")
rpn = importlib.import_module("3dal_pytorch_amd.rpn")
sparse = importlib.import_module("3dal_pytorch_amd.sparse")
detector = importlib.import_module("3dal_pytorch_amd.detector")
two_stage = importlib.import_module("3dal_pytorch_amd.two_stage")
KEYS = ("bev",) + S.LEVELS
_CASE = {}


def case(prec, fault=None, c_in=5):
    """the model's backbone on sparse_ref.backbone_case(c_in), computed once"""
    key = (prec, fault, c_in)
    if key not in _CASE:
        feats, idx, B, shape = S.backbone_case(c_in)
        if prec == "truth":
            _CASE[key] = S.backbone(S.Dense(B), S.backbone_weights(c_in), feats, idx, shape)
        elif prec == "yardstick":
            _CASE[key] = S.backbone(S.Dense(B, torch.float32), S.backbone_weights(c_in), feats, idx, shape)
        else:
            _CASE[key] = L.backbone(S.backbone_weights(c_in), feats, idx, shape, prec, fault, B=B)
    return _CASE[key]


@pytest.mark.parametrize("c_in", (5, 6))
def test_the_f64_mode_is_sparse_refs_backbone(c_in):
    truth, got = case("truth", c_in=c_in), case("f64", c_in=c_in)
    assert list(got) == list(truth)
    for k in truth:
        assert got[k].dtype == np.float64 and np.array_equal(got[k], truth[k]), k


def test_the_model_has_resolution():
    truth, yard = case("truth"), case("yardstick")
    for k in KEYS:
        y, e16, eb16 = L.errors(yard[k], truth[k]), L.errors(case("fp16")[k], truth[k]), L.errors(case("bf16")[k], truth[k])
        print(f"{k:6s} rms: yardstick {y['rms']:.3e}  fp16 {e16['rms']:.3e}  bf16 {eb16['rms']:.3e}  bf16 / fp16 {eb16['rms'] / e16['rms']:.2f}")
        assert e16["rms"] >= 100 * y["rms"], k
        assert 4 * e16["rms"] <= eb16["rms"] <= 16 * e16["rms"], k


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_planted_faults_move_the_chain(prec):
    truth = case("truth")
    for k in KEYS:
        model = case(prec)[k]
        base = L.errors(model, truth[k])
        ratio, moved = {}, {}
        for f in L.FAULTS:
            got = case(prec, f)[k]
            ratio[f] = L.errors(got, truth[k])["rms"] / base["rms"]
            d = np.abs(got - model)
            moved[f] = (float(np.sqrt((d ** 2).mean()) / np.sqrt((truth[k] ** 2).mean())) / base["rms"],
                        float(d.max() / np.abs(truth[k]).max()) / base["max"])
            print(f"{k:6s} {prec} {f:18s} rms error x {ratio[f]:.3f}   distance from the model: rms {moved[f][0]:.3f}  max {moved[f][1]:.3f} "
                  "of the model's error")
        assert ratio["truncate"] >= 2.0, (k, ratio)
        assert 0.6 <= ratio["weights_unrounded"] <= 0.85 and 0.6 <= ratio["inputs_unrounded"] <= 0.85, (k, ratio)
        for f in L.FAULTS:
            assert moved[f][0] >= RMS_SLACK - 1, (k, f, moved[f])


@pytest.mark.parametrize("c_in", (5, 6))
def test_every_layers_input_stays_an_eighth_of_fp16s_range(c_in):
    feats, idx, B, shape = S.backbone_case(c_in)
    peak = L.inner_peak(S.backbone_weights(c_in), feats, idx, shape, B)
    print(f"c_in {c_in}: the largest input of any layer in the float64 chain is {peak:.1f}")
    assert 0 < peak < 2.0 ** 13
    if c_in == 5:
        tops = [float(np.abs(case("truth")[k]).max()) for k in S.LEVELS + ("bev",)]
        assert [round(t) for t in tops] == [24, 87, 421, 1172, 1547], tops


def test_a_single_layer_of_the_model_rounds_inputs_and_weights_only():
    shape, B = (5, 7, 9), 1
    idx = S.unkey(np.arange(int(np.prod(shape))), shape)
    w, b, bn = S.layer_weights("lp/cpu/layer", (3, 3, 3), 16, 16, True, True)
    feats = S.synth.uniform(S.SEED, "lp/cpu/x", (idx.shape[0], 16), 0.0, 2.0).astype(np.float32)
    args = (feats, idx, shape, w, b, bn, (3, 3, 3), (1, 1, 1), (1, 1, 1), True, True)
    assert np.array_equal(L.layer(S.Dense(B), *args, "f64", residual=True), S.layer(S.Dense(B), *args, True))
    wf, bf = S.fold(w, b, bn)
    for prec in ("fp16", "bf16"):
        got = L.layer(S.Dense(B), *args, prec, residual=True)
        # the same thing by hand: rounded operands through sparse_ref's own layer, then the unrounded residual
        lin = S.layer(S.Dense(B), L.q(feats, prec), idx, shape, L.q(wf, prec), bf, None, (3, 3, 3), (1, 1, 1), (1, 1, 1), True, False)
        dense_x = np.zeros((B, 16, *shape))
        dense_x[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]] = feats
        assert np.array_equal(got, np.maximum(lin + dense_x, 0.0))
        assert not np.array_equal(got, L.layer(S.Dense(B), *args, prec, residual=True, fault="residual_rounded"))


# ------------------------------------------------------------------------------------- the plumbing
PP_MODEL = dict(reader=dict(type="PillarFeatureNet", num_filters=[64, 64], num_input_features=5, with_distance=False,
                            voxel_size=(0.32, 0.32, 6.0), pc_range=(0.0, -5.76, -2.0, 14.08, 5.76, 4.0)),
                backbone=dict(type="PointPillarsScatter", ds_factor=1),
                neck=dict(type="RPN", layer_nums=[3], ds_layer_strides=[1], ds_num_filters=[64], us_layer_strides=[1], us_num_filters=[64],
                          num_input_features=64),
                bbox_head=dict(type="CenterHead", in_channels=64, tasks=[dict(num_class=1, class_names=["VEHICLE"])], dataset="waymo",
                               weight=2, code_weights=[1.0] * 8, common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2)}))
VN_MODEL = dict(PP_MODEL, reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5),
                backbone=dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8),
                neck=dict(PP_MODEL["neck"], num_input_features=256))


def _sparse_modules(m):
    return [c for c in m.modules() if isinstance(c, sparse._SparseLayers)]


def test_sparse_precision_is_validated_everywhere_and_reaches_the_children():
    import roi_ref
    conv, block, bb = sparse.SubMConv3d(16, 16, 3), sparse.SparseBasicBlock(16, 16), sparse.SpMiddleResNetFHD(num_input_features=5)
    vn = detector.VoxelNet(**VN_MODEL)
    ts = two_stage.TwoStageDetector(dict(type="VoxelNet", **VN_MODEL),
                                    [dict(type="BEVFeatureExtractor", pc_start=[0.0, -5.76], voxel_size=[0.32, 0.32], out_stride=8)],
                                    dict(type="RoIHead", input_channels=320, model_cfg=roi_ref.PRODUCTION, code_size=7), 100)
    for m in (conv, block, bb, vn, ts):
        assert m.sparse_precision == "fp32"
        for bad, why in (("f16x3", "point heads only"), ("fp64", "unknown precision"), (None, "unknown precision"), ("FP16", "unknown")):
            with pytest.raises(ValueError, match=why):
                m.sparse_precision = bad
            assert m.sparse_precision == "fp32"
        for ok in ("fp16", "bf16", "fp32"):
            m.sparse_precision = ok
            assert m.sparse_precision == ok
    assert len(_sparse_modules(bb)) == 1 + 5 + 8 * 3          # the backbone, its five stems, eight blocks of two layers
    bb.sparse_precision = "bf16"
    assert all(c.sparse_precision == "bf16" for c in _sparse_modules(bb))
    block.sparse_precision = "fp16"
    assert block.conv1.sparse_precision == block.conv2.sparse_precision == "fp16"
    bb.conv2[3].sparse_precision = "fp16"                     # a child alone: its own layers, not its parent
    assert bb.conv2[3].conv2.sparse_precision == "fp16" and bb.sparse_precision == bb.conv2[4].sparse_precision == "bf16"
    ts.sparse_precision = "fp16"
    assert ts.single_det.sparse_precision == ts.single_det.backbone.sparse_precision == "fp16"
    assert all(c.sparse_precision == "fp16" for c in _sparse_modules(ts))
    assert not hasattr(vn.backbone, "precision") and not hasattr(vn.reader, "sparse_precision") and not hasattr(vn.neck, "sparse_precision")
    assert "sparse_precision" not in "".join(bb.state_dict())
    for bad in ("f16x3", "int8"):
        with pytest.raises(ValueError):
            sparse.pack_layer(conv, None, precision=bad)
        with pytest.raises(ValueError):
            sparse.conv(torch.zeros(4, 16), torch.zeros((27, 4), dtype=torch.int32), None, torch.zeros(4), 16, 16, None, precision=bad)
    with pytest.raises(ValueError, match="16-bit"):
        sparse.conv(torch.zeros(4, 16), torch.zeros((27, 4), dtype=torch.int32), None, torch.zeros(4), 16, 16, None, out16=True)


def test_the_two_knobs_do_not_touch_each_other_and_pointpillars_refuses():
    vn, pp = detector.VoxelNet(**VN_MODEL), detector.PointPillars(**PP_MODEL)
    vn.precision = "fp16"
    assert vn.sparse_precision == vn.backbone.sparse_precision == "fp32" and vn.neck.precision == "fp16"
    vn.sparse_precision = "bf16"
    assert vn.precision == vn.neck.precision == vn.bbox_head.precision == "fp16" and vn.backbone.sparse_precision == "bf16"
    vn.precision = "fp32"
    assert vn.sparse_precision == "bf16"
    assert pp.sparse_precision == "fp32"
    for value in ("fp16", "fp32"):
        with pytest.raises(ValueError, match="no sparse convolutions"):
            pp.sparse_precision = value
    with pytest.raises(ValueError, match="unknown precision"):
        pp.sparse_precision = "fp64"
    assert pp.precision == "fp32" and not hasattr(pp.backbone, "sparse_precision")


def test_the_cache_key_changes_with_sparse_precision(monkeypatch):
    calls = []

    def fake_pack(conv, bn, status=None, precision="fp32"):
        calls.append((conv.out_channels, precision))
        return torch.zeros(8, dtype=torch.float32 if precision == "fp32" else torch.uint8)

    monkeypatch.setattr(sparse, "pack_layer", fake_pack)
    bb = sparse.SpMiddleResNetFHD(num_input_features=5).eval()
    for m, n_layers in ((bb, 5), (bb.conv3[3], 2), (bb.conv2[0], 1)):
        calls.clear()
        bb.sparse_precision = "fp32"
        a = m.packed()
        assert m.packed() is a and len(calls) == n_layers and {p for _, p in calls} == {"fp32"}
        bb.sparse_precision = "fp16"                                  # set on the container: the child repacks
        b = m.packed()
        assert b is not a and m.packed() is b and len(calls) == 2 * n_layers and calls[-1][1] == "fp16" and b[0].dtype == torch.uint8
        bb.sparse_precision = "fp16"                                  # the same value: no repack
        assert m.packed() is b
        bb.sparse_precision = "bf16"
        c = m.packed()
        assert c is not b and len(calls) == 3 * n_layers and calls[-1][1] == "bf16"
        bb.sparse_precision = "fp32"
        assert m.packed() is not c and len(calls) == 4 * n_layers and calls[-1][1] == "fp32"
    # train mode ignores it: the differentiable route packs the raw weight as float32 whatever the knob says, and the
    # eval-mode forward is refused in train mode in every precision
    bb.sparse_precision = "fp16"
    calls.clear()
    sparse._pack_raw(bb.conv1[0].conv1.weight, None, (3, 3, 3))
    assert calls == [(16, "fp32")]
    with pytest.raises(RuntimeError, match="eval-mode"):
        bb.train()(torch.zeros(1, 5), torch.zeros((1, 4), dtype=torch.int32), 1, [4, 4, 8])


def test_features16_is_checked_and_like_does_not_invent_it(monkeypatch):
    monkeypatch.setattr(hip, "require_gpu", lambda t, what: None)
    f, i = torch.zeros(6, 16), torch.zeros((6, 4), dtype=torch.int32)
    x = sparse.SparseConvTensor(f, i, (4, 4, 4), 1)
    assert x.features16 is None and x.capacity == 6
    for dt in (torch.float16, torch.bfloat16):
        y = sparse.SparseConvTensor(f, i, (4, 4, 4), 1, features16=f.to(dt))
        assert y.features16.dtype == dt and y.like(f).features16 is None and y.like(f, f.to(dt)).features16 is not None
    only16 = sparse.SparseConvTensor(None, i, (4, 4, 4), 1, features16=f.half())
    assert only16.features is None and only16.capacity == 6
    for bad in (f, f.double(), f.half()[:5], f.half()[:, :8]):
        with pytest.raises(ValueError, match="features16"):
            sparse.SparseConvTensor(f, i, (4, 4, 4), 1, features16=bad)
    with pytest.raises(TypeError):
        sparse.SparseConvTensor(None, i, (4, 4, 4), 1)


def test_the_new_entries_are_bound():
    for name in ("dal3_sp_conv_lp_pack_bytes", "dal3_sp_conv_lp_pack", "dal3_sp_conv_lp"):
        assert name in hip.SIGNATURES, name
    fields = [f[0] for f in hip.SpConvLpArgs._fields_]
    assert fields[:len(hip.SpConvArgs._fields_)] == [f[0] for f in hip.SpConvArgs._fields_] and fields[-3:] == ["dtype", "x16", "y16"]
    assert hip.SpConvLpArgs.__doc__.startswith("dal3_sp_conv_lp_args")
