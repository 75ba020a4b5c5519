"""The detector's dense stage on 16-bit MFMA operands (dal3_conv2d_lp_pack / dal3_conv2d_lp; `precision` of rpn.RPN,
rpn.CenterHead and the detector classes), for "fp16" and "bf16":

  impulses      bit for bit: a unit impulse lands as relu(fl32(q(W')[tap] + b')), which pins the tap orientation, the padding,
                the stride-2 phase, the transposed forms' sub-positions, the channel slice and the weight rounding; impulses
                just above a rounding tie and on ties whose even neighbour is below / above pin the activation rounding
                (q(x) q(W') has at most 22 significant bits: exact in float32, so fl32(q(x) q(W') + b') is the one value).
  single layers against the float64 evaluation of the ROUNDED operands, under the fp32 kernel's own bars (rpn_ref.BARS) with
                the torch-CPU fp32 layer on the same rounded operands as the yardstick: what is left is the fp32 accumulation.
                Channel pairs of the issue plus the seam of the kernel's staged channel chunk, which is 32 input channels
                for stride 1 (3x3, 1x1, transposed) and 16 for the 3x3 of stride 2: c_in 31 | 33 and 15 | 17.
  neck and head against tests/rpn_lp_model.py: error against the unrounded float64 truth <= emu16.RMS_SLACK x the model's
                (per-tensor rms) and <= emu16.MODEL_SLACK x (maxima).
  grid, cache, fused head launches, the detector door and the refusals.

With DAL3_RPN_LP_RECORD=<path> every error and ratio is written to <path> (how profiles/rpn_lp_measured.json was made)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import rpn_gpu
import rpn_lp_model as M
import rpn_ref as R
from emu16 import MODEL_SLACK, RMS_SLACK
from rpn_gpu import KINDS, _dev, _hold, dense_case, head_module, layer_params, neck_module, rpn, torch_layer, yardstick
from test_gpu_rpn import FORMS, IMPULSE, SCHEDULE, SENTINEL, _impulse_expected, _view

hip = rpn_gpu.hip
pytestmark = pytest.mark.gpu

PRECS = ("fp16", "bf16")
TIES = {"fp16": (1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11),
        "bf16": (1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8)}
_LP_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _lp_record_file():
    yield
    path = os.environ.get("DAL3_RPN_LP_RECORD")
    if path:
        rows = dict(_LP_RECORD, **{k: v for k, v in rpn_gpu._RECORD.items() if k.startswith("lp/")})
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(rows, f, indent=1, sort_keys=True)


@torch.no_grad()
def lp_pack(w, b, bn, eps, kind, stride, prec):
    conv, norm = torch_layer(w, b, bn, eps, kind, stride, "cuda")
    return rpn.pack_layer(conv, norm, KINDS[kind, stride], precision=prec, name="the test's layer"), conv.out_channels


@torch.no_grad()
def lp_run(x_dev, pack, kind, stride, relu, prec, **kw):
    return rpn.conv2d(x_dev, pack[0], KINDS[kind, stride], stride, relu, pack[1], precision=prec, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------- impulses
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind,stride", FORMS)
def test_impulses_are_bit_exact(kind, stride, prec):
    I = IMPULSE
    w, b, bn = layer_params(f"impulse/{kind}{stride}", kind, stride, I["c_in"], I["c_out"], True, True)
    wf, bf = R.fold(w, b, bn, R.NECK_EPS, deconv=kind == "deconv")
    wq = M.q(wf, prec)
    assert (wq != wf).mean() > 0.9 and (bf < 0).any() and (bf > 0).any()
    pack = lp_pack(w, b, bn, R.NECK_EPS, kind, stride, prec)
    H, W = I["H"], I["W"]
    spots = [(y, x) for y in (0, H // 2, H - 1) for x in (0, W // 2, W - 1)]       # corners, edges, the interior
    spots += [(7, 31), (8, 32)]                                                      # either side of the tile seams
    x = torch.zeros((I["B"], I["c_in"], H, W), device="cuda")

    def check(b0, c0, y0, x0, value, relu):
        # q(value) q(W') is exact in float32; the kernel's chunk sum holds it alone, and the total is one fp32 addition
        scaled = (M.q(np.float32(value), prec) * wq).astype(np.float32)
        assert np.array_equal(scaled.astype(np.float64), M.q(np.float32(value), prec).astype(np.float64) * wq.astype(np.float64))
        want = _impulse_expected(scaled, bf, kind, stride, b0, c0, y0, x0, relu)
        x.zero_()
        x[b0, c0, y0, x0] = value
        out = torch.full((I["B"], I["channels"]) + want.shape[2:], SENTINEL, device="cuda")
        y = lp_run(x, pack, kind, stride, relu, prec, out=out, channel_offset=I["offset"])
        got = out.cpu().numpy()
        assert y.data_ptr() == out[:, I["offset"]:].data_ptr()
        mine = got[:, I["offset"]:I["offset"] + I["c_out"]]
        d = np.argwhere(_bits(mine) != _bits(want))
        assert not len(d), ((b0, c0, y0, x0, value, relu), len(d), [(tuple(i), float(mine[tuple(i)]), float(want[tuple(i)])) for i in d[:3]])
        rest = np.delete(got, np.s_[I["offset"]:I["offset"] + I["c_out"]], axis=1)
        assert (rest == SENTINEL).all(), "a channel outside the slice was written"
        return want

    n = 0
    for b0 in range(I["B"]):
        for c0 in (0, I["c_in"] - 1):
            for y0, x0 in spots:
                check(b0, c0, y0, x0, 1.0, True)
                n += 1
    assert n == 2 * 2 * 11
    # the activation rounding: just above a tie (up), a tie whose even neighbour is below (down), one whose is above (up)
    up, down, up2 = (float(M.q(np.float32(v), prec)[0]) for v in TIES[prec])
    ulp = 2.0 ** -10 if prec == "fp16" else 2.0 ** -7
    assert (up, down, up2) == (1 + ulp, 1.0, 1 + 2 * ulp)
    for i, v in enumerate(TIES[prec]):
        check(i % 2, 16 + i, 3 + i, 30 + i, v, True)
        check(1, 8 + i, H - 1, W - 1 - i, -v, False)
    # without ReLU the negative values come through
    want = check(1, 0, H - 1, W - 1, 1.0, False)
    assert (want < 0).any()


# ------------------------------------------------------------------------------------- single layers
PAIRS = ((20, 33), (24, 40), (64, 64), (128, 256), (384, 64), (64, 3), (31, 40), (33, 40), (15, 40), (17, 40))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", range(len(SCHEDULE)))
@pytest.mark.parametrize("c_in,c_out", PAIRS)
def test_single_layers_under_the_fp32_kernels_bars(c_in, c_out, case, prec):
    (H, W), B, kind, stride, relu, bias, bn_on, how, wg = SCHEDULE[case]
    tag = f"layer/{c_in}-{c_out}/{kind}{stride}/{H}x{W}"
    w, b, bn = layer_params(tag, kind, stride, c_in, c_out, bias, bn_on)
    x = R.synth.uniform(R.SEED, tag + "/x", (B, c_in, H, W), 0.0, 2.0).astype(np.float32)
    x *= R.synth.uniform(R.SEED, tag + "/live", (B, 1, H, W)) < 0.6
    eps = R.NECK_EPS if kind != "3x3" or stride == 2 else R.HEAD_EPS
    wf, bf = R.fold(w, b, bn, eps, deconv=kind == "deconv")
    xq, wq = M.q(x, prec), M.q(wf, prec)
    truth = R.folded_layer(xq, wq, bf, kind, stride, relu)
    f32 = yardstick(xq, wq, bf, None, eps, kind, stride, relu)
    got = lp_run(_view(x, how), lp_pack(w, b, bn, eps, kind, stride, prec), kind, stride, relu, prec, max_workgroups=wg).cpu().numpy()
    assert got.shape == truth.shape == f32.shape
    _hold(f"lp/{prec}/{tag}/wg{wg}", got, f32, truth)


# ------------------------------------------------------------------------------------- the whole neck and head
_MODEL = {}


def model_case(tag, prec):
    """the model's (neck, head, head alone on the yardstick's neck output) on canvas `tag`, computed once"""
    if (tag, prec) not in _MODEL:
        x, _, n32, _, _ = dense_case(tag)
        n = M.neck(R.neck_weights(), x, prec)
        _MODEL[tag, prec] = (n, R.head_cat(M.head(R.head_weights(), n, prec)), R.head_cat(M.head(R.head_weights(), n32, prec)))
    return _MODEL[tag, prec]


def hold_chain(row, got, model, truth):
    """the chain bar: the kernel's error against the unrounded float64 truth over the model's error against it"""
    e, m = M.errors(got, truth), M.errors(model, truth)
    ratio = {k: e[k] / m[k] for k in e}
    _LP_RECORD[row] = {"measured": e, "model": m, "ratio": ratio}
    for k, slack in (("rms", RMS_SLACK), ("max", MODEL_SLACK)):
        print(f"{row:30s} {k:4s} {e[k]:10.3e}  model {m[k]:10.3e}  ratio {ratio[k]:6.3f}  slack {slack:g}")
    assert ratio["rms"] <= RMS_SLACK and ratio["max"] <= MODEL_SLACK, (row, ratio)


def _cat(preds):
    return R.head_cat([{k: v.cpu().numpy() for k, v in d.items()} for d in preds])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tag", ["a", "b", "big"])
def test_whole_neck_and_head_against_the_model(tag, prec):
    x, n64, n32, h64, h32 = dense_case(tag)
    neck, head = neck_module(), head_module()
    neck.precision = head.precision = prec
    assert neck.hip_serves() and head.hip_serves()
    with torch.no_grad():
        n = neck(_dev(x))
        preds = head(n)
        alone = head(_dev(n32))
    assert n.shape == n64.shape and n.is_contiguous() and n.dtype == torch.float32
    got_n = n.cpu().numpy()
    for c in (R.DEAD_CHANNEL, 128 + R.DEAD_CHANNEL, 256 + R.DEAD_CHANNEL):
        assert not n64[:, c].any() and not got_n[:, c].any() and not np.signbit(got_n[:, c]).any()
    m_n, m_h, m_alone = model_case(tag, prec)
    hold_chain(f"lp/{prec}/neck/{tag}", got_n, m_n, n64)
    assert list(preds[0]) == list(R.HEAD_ORDER) and [preds[0][k].shape[1] for k in R.HEAD_ORDER] == [2, 1, 3, 2, 3]
    hold_chain(f"lp/{prec}/head/{tag}", _cat(preds), m_h, h64)
    h64_alone = R.head_cat(R.head_f64(R.head_weights(), n32))
    hold_chain(f"lp/{prec}/head_alone/{tag}", _cat(alone), m_alone, h64_alone)


# ------------------------------------------------------------------------------------- grid and cache
@pytest.mark.parametrize("prec", PRECS)
def test_grid_cache_and_the_precision_switch(prec):
    x = dense_case("a")[0]
    neck = neck_module()
    with torch.no_grad():
        f32 = neck(_dev(x)).cpu().numpy()
        neck.precision = prec
        a = neck(_dev(x)).cpu().numpy()
        b = neck(_dev(x), max_workgroups=3).cpu().numpy()
        assert np.array_equal(_bits(a), _bits(b)) and not np.array_equal(a, f32)
        packed = neck.packed()
        assert neck.packed() is packed and packed[0].dtype == torch.uint8
        neck.blocks[0][1].weight.mul_(2.0)                      # a version bump: the cache is rebuilt
        assert neck.packed() is not packed
        assert not np.array_equal(a, neck(_dev(x)).cpu().numpy())
        neck.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in R.neck_weights().items()})
        assert np.array_equal(_bits(neck(_dev(x)).cpu().numpy()), _bits(a))
        neck.precision = "fp32"
        assert neck.packed()[0].dtype == torch.float32
        assert np.array_equal(_bits(neck(_dev(x)).cpu().numpy()), _bits(f32))
    neck.precision = prec
    assert neck.train().composite(_dev(x)).shape == a.shape     # train mode is the composite, whatever the precision


@pytest.mark.parametrize("prec", PRECS + ("fp32",))
def test_fused_and_unfused_head_launches_give_the_same_bits(prec):
    n32 = dense_case("b")[2]
    head = head_module()
    head.precision = prec
    with torch.no_grad():
        assert head.packed()[1][0] is not None
        fused = _cat(head(_dev(n32)))
        head._fusable = lambda task: False
        head.invalidate_packed()
        assert head.packed()[1][0] is None
        assert np.array_equal(_bits(_cat(head(_dev(n32)))), _bits(fused))
    # a 32-channel head is unfused by construction: the module's maps are the layers run one by one
    narrow = rpn.CenterHead(**R.HEAD)
    for name in narrow.tasks[0].heads:
        seq = rpn.SepHead(64, {name: narrow.tasks[0].heads[name]}, head_conv=32, bn=True, final_kernel=3)
        setattr(narrow.tasks[0], name, getattr(seq, name))
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for p in narrow.parameters():
            p.copy_((torch.rand(p.shape, generator=g) - 0.5) * (0.2 if p.dim() > 1 else 1.0))
    narrow = narrow.cuda().eval()
    narrow.precision = prec
    assert not narrow._fusable(narrow.tasks[0]) and narrow.hip_serves()
    with torch.no_grad():
        got = narrow(_dev(n32))[0]

        def one(seq, x):
            for conv, bn, relu in rpn._split(seq):
                kind, stride = rpn.layer_kind(conv)
                x = rpn.conv2d(x, rpn.pack_layer(conv, bn, kind, precision=prec), kind, stride, relu, conv.out_channels, precision=prec)
            return x

        mid = one(narrow.shared_conv, _dev(n32))
        for name in narrow.tasks[0].heads:
            assert torch.equal(got[name], one(getattr(narrow.tasks[0], name), mid)), name


# ------------------------------------------------------------------------------------- the detector door
def _structure(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y) == {"box3d_lidar", "scores", "label_preds", "metadata"}
        for k in ("box3d_lidar", "scores", "label_preds"):
            assert x[k].dtype == y[k].dtype and x[k].device == y[k].device and x[k].shape[1:] == y[k].shape[1:], k
        assert x["metadata"] is y["metadata"]
    assert sum(int(x["scores"].numel()) for x in a) > 0 and sum(int(y["scores"].numel()) for y in b) > 0


def test_pointpillars_door():
    import test_gpu_detector as PP
    pillars = importlib.import_module("3dal_pytorch_amd.pillars")
    m = PP.detector.PointPillars(**PP.MODEL, test_cfg=PP.TEST_CFG, max_points=20, max_voxels=2000)
    m.load_state_dict(PP.checkpoint(), strict=True)
    m = m.cuda().eval()
    pts, off = PP.sweep()
    dpts = _dev(pts)
    want = m.detect(dpts, off, metadata=PP.META)
    r = pillars.voxelize(dpts, off, PP.VOXEL, PP.RANGE, 20, 2000)
    canvas = m.reader.forward_canvas(r.voxels, r.num_points, r.coordinates, 2, [44, 36], n_pillars=r.n_pillars)
    x = canvas.cpu().numpy()
    n64 = R.neck_f64(R.neck_weights(), x)
    h64 = R.head_cat(R.head_f64(R.head_weights(), n64))
    m.precision = "fp16"
    assert m.neck.precision == m.bbox_head.precision == "fp16"
    _structure(m.detect(dpts, off, metadata=PP.META), want)
    assert torch.equal(m.reader.forward_canvas(r.voxels, r.num_points, r.coordinates, 2, [44, 36], n_pillars=r.n_pillars), canvas)
    with torch.no_grad():
        n = m.neck(canvas)
        preds = m.bbox_head(n)
    m_n = M.neck(R.neck_weights(), x, "fp16")
    hold_chain("lp/fp16/pointpillars/neck", n.cpu().numpy(), m_n, n64)
    hold_chain("lp/fp16/pointpillars/head", _cat(preds), R.head_cat(M.head(R.head_weights(), m_n, "fp16")), h64)
    m.precision = "fp32"
    got = m.detect(dpts, off, metadata=PP.META)
    assert all(torch.equal(g[k], w[k]) for g, w in zip(got, want) for k in ("box3d_lidar", "scores", "label_preds"))


def test_voxelnet_door():
    import test_gpu_voxelnet as V
    pillars = importlib.import_module("3dal_pytorch_amd.pillars")
    m = V.detector.VoxelNet(**V.MODEL, test_cfg=V.TEST_CFG, **V.KW)
    m.load_state_dict(V.checkpoint(), strict=True)
    m = m.cuda().eval()
    pts, off = V.sweep()
    dpts = _dev(pts)
    want = m.detect(dpts, off, metadata=V.META)
    r = pillars.voxelize(dpts, off, V.VOXEL, V.RANGE, 5, 4000)
    voxels, coords, num, nv = r.finish()

    def stages():
        with torch.no_grad():
            bev, _ = m.backbone(m.reader(voxels, num), coords, 2, V.GRID)
            n = m.neck(bev)
            return bev, n, m.bbox_head(n)

    bev, n, preds = stages()
    m.precision = "fp16"
    assert m.neck.precision == m.bbox_head.precision == "fp16" and not hasattr(m.backbone, "precision")
    _structure(m.detect(dpts, off, metadata=V.META), want)
    bev16, n16, preds16 = stages()
    assert torch.equal(bev16, bev)                                    # the reader and the sparse middle are untouched
    assert not torch.equal(n16, n)
    # the chain bar, with the truth and the model chained over THIS detector's neck and head from its own state dict
    sd = {k: v.cpu().numpy() for k, v in m.state_dict().items()}
    nsd = {k[len("neck."):]: v for k, v in sd.items() if k.startswith("neck.")}
    hsd = {k[len("bbox_head."):]: v for k, v in sd.items() if k.startswith("bbox_head.")}
    cfg, x = V.MODEL["neck"], bev.cpu().numpy()
    n64, m_n = M.neck(nsd, x, "f64", cfg=cfg), M.neck(nsd, x, "fp16", cfg=cfg)
    assert n64.shape == tuple(n.shape) and np.abs(n64).max() > 0
    hold_chain("lp/fp16/voxelnet/neck", n16.cpu().numpy(), m_n, n64)
    hold_chain("lp/fp16/voxelnet/head", _cat(preds16), R.head_cat(M.head(hsd, m_n, "fp16")), R.head_cat(M.head(hsd, n64, "f64")))
    m.neck.precision = "fp32"                                         # the head alone on 16-bit operands
    with torch.no_grad():
        n_again = m.neck(bev)
        assert torch.equal(n_again, n)
        only_head = m.bbox_head(n_again)
    for k in preds[0]:
        assert not torch.equal(only_head[0][k], preds[0][k]), k
    n32 = n.cpu().numpy()
    hold_chain("lp/fp16/voxelnet/head_alone", _cat(only_head), R.head_cat(M.head(hsd, n32, "fp16")), R.head_cat(M.head(hsd, n32, "f64")))


# ------------------------------------------------------------------------------------- refusals
def test_a_weight_beyond_fp16_is_refused_at_pack_time_by_name():
    neck = neck_module()
    with torch.no_grad():
        neck.blocks[1][4].weight[3, 2, 1, 1] = 1.0e6
    neck.precision = "fp16"
    with pytest.raises(ValueError, match=r"blocks\.1\.4.*fp16's range"):
        neck(_dev(dense_case("a")[0]))
    neck.precision = "bf16"                                            # bf16 has float32's range
    with torch.no_grad():
        assert torch.isfinite(neck(_dev(dense_case("a")[0]))).all()
    conv, bn = neck.blocks[1][4], neck.blocks[1][5]
    with pytest.raises(ValueError, match="the layer"):
        rpn.pack_layer(conv, bn, hip.CONV2D_3X3, precision="fp16")


def test_a_wrong_dtype_is_einval_and_nothing_is_launched():
    lib = hip.lib()
    w, b, bn = layer_params("refusal", "3x3", 1, 24, 40, True, True)
    pack, c_out = lp_pack(w, b, bn, R.NECK_EPS, "3x3", 1, "fp16")
    x = torch.ones((1, 24, 5, 7), device="cuda")
    out = torch.full((1, 40, 5, 7), SENTINEL, device="cuda")
    for dtype in (hip.F32, hip.F16X3, 7, -1):
        a = hip.Conv2dLpArgs(kind=hip.CONV2D_3X3, stride=1, relu=1, c_in=24, c_out=40, y_channels=40, y_channel_offset=0,
                             max_workgroups=0, dtype=dtype, B=1, H=5, W=7, x=hip.nchw_map(x), y=hip.nchw_map(out), packed=hip.ptr(pack))
        assert lib.dal3_conv2d_lp(a, hip.stream()) == hip.EINVAL and b"dtype" in lib.dal3_last_error()
        conv, norm = torch_layer(w, b, bn, R.NECK_EPS, "3x3", 1, "cuda")
        buf = torch.full((pack.numel(),), 0x5A, dtype=torch.uint8, device="cuda")
        L = hip.fold_layer_struct(conv, norm)
        assert lib.dal3_conv2d_lp_pack(L, hip.CONV2D_3X3, R.NECK_EPS, dtype, hip.ptr(buf), hip.stream()) == hip.EINVAL
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((buf == 0x5A).all())
    assert lib.dal3_conv2d_lp_pack_bytes(hip.CONV2D_3X3, 24, 40) == pack.numel() == 2 * 32 * 4 + 2 * 2 * 9 * 1024
    assert lib.dal3_conv2d_lp_pack_bytes(9, 24, 40) == 0 and lib.dal3_conv2d_lp_pack_bytes(hip.CONV2D_3X3, 0, 40) == 0
    with pytest.raises(ValueError, match="not those of"):
        rpn.conv2d(x, pack, hip.CONV2D_3X3, 1, True, 40)               # a 16-bit blob given to the fp32 door
