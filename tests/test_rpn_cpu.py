"""CPU-side checks of the detector's dense stage (3dal_pytorch_amd/rpn.py, detector.py; dal3_conv2d_pack / dal3_conv2d):
the float64 restatement of tests/rpn_ref.py against what the reference's own RPN and CenterHead recorded (tests/golden/
rpn.npz, written by tests/golden/gen_rpn.py), the planted faults against the GPU tests' bars, the modules' keys against the
reference's, the stock-torch composite against the recorded fp32 outputs bit for bit, the C ABI's declarations
and argument checks, and the FLOP count of tools/bench_detector.py. No GPU compute here."""
import ctypes
import importlib
import importlib.util
import os
import zlib

import numpy as np
import pytest
import torch

import rpn_ref as R
from _common import ROOT, golden

hip = importlib.import_module("3dal_pytorch_amd._hip")
rpn = importlib.import_module("3dal_pytorch_amd.rpn")
detector = importlib.import_module("3dal_pytorch_amd.detector")

ENTRIES = ("dal3_conv2d_pack_floats", "dal3_conv2d_pack", "dal3_conv2d")
MODEL = dict(reader=dict(type="PillarFeatureNet", num_filters=[64, 64], num_input_features=5, with_distance=False,
                         voxel_size=(0.32, 0.32, 6.0), pc_range=(-74.88, -74.88, -2, 74.88, 74.88, 4.0)),
             backbone=dict(type="PointPillarsScatter", ds_factor=1), neck=dict(type="RPN", **R.NECK),
             bbox_head=dict(type="CenterHead", **R.HEAD))
# the smallest ratio a planted fault reached over the three measures, the two canvases and neck / head (printed by
# test_planted_faults_exceed_ten_times_the_largest_bar): the bars of rpn_ref.BARS stay under a tenth of it
SMALLEST_FAULT_RATIO = 3.5e2


def _truth(g, tag, name):
    return g[f"{tag}_{name}_f32"].astype(np.float64) + g[f"{tag}_{name}_diff"].astype(np.float64)


def _canvas(g, tag):
    x = R.canvas(tag, R.CANVASES[tag])
    assert abs(float(x.astype(np.float64).sum()) - float(g[f"{tag}_in_sum"])) < 1e-9, "the seeded canvas drifted from the fixture"
    return x


@pytest.fixture(scope="module")
def restated():
    """tag -> (x, neck f64 (all channels), head f64): computed once, shared, read-only"""
    g, out = golden("rpn"), {}
    for tag in R.CANVASES:
        x = _canvas(g, tag)
        n = R.neck_f64(R.neck_weights(), x)
        out[tag] = (x, n, R.head_cat(R.head_f64(R.head_weights(), n)))
        for a in out[tag]:
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("tag", list(R.CANVASES))
def test_restatement_equals_the_references_float64_outputs(tag, restated):
    g = golden("rpn")
    x, n, h = restated[tag]
    assert 0.2 < float(g[f"{tag}_occupied"]) < 0.35 and abs(float((x != 0).any(1).mean()) - float(g[f"{tag}_occupied"])) < 1e-12
    for name, mine in (("neck", n[:, ::4]), ("head", h)):
        want = _truth(g, tag, name)
        assert mine.shape == want.shape
        assert np.abs(mine - want).max() <= 1e-12 * np.abs(want).max(), name
        y = R.judge(g[f"{tag}_{name}_f32"], want)
        assert y["dead_ok"] and 1e-8 < y["tensor"] < 1e-5, y        # the yardstick is fp32 rounding, neither 0 nor a bug
    for c in (R.DEAD_CHANNEL, 128 + R.DEAD_CHANNEL, 256 + R.DEAD_CHANNEL):
        assert not n[:, c].any()


def test_planted_faults_exceed_ten_times_the_largest_bar(restated):
    g, smallest = golden("rpn"), np.inf
    bar = max(R.BARS.values())
    for tag in R.CANVASES:
        x, n, h = restated[tag]
        for fault in R.FAULTS:
            fn = R.neck_f64(R.neck_weights(), x, fault=fault)
            fh = R.head_cat(R.head_f64(R.head_weights(), fn if fault in R.FAULTS[:5] else n, fault=fault))
            # a fault shows where it acts: the neck's in the neck's output (and through it in the head's), the head's in the head's
            where = (("neck", fn[:, ::4]), ("head", fh)) if fault in R.FAULTS[:5] else (("head", fh),)
            for name, out in where:
                ratio = R.ratios(out, g[f"{tag}_{name}_f32"], _truth(g, tag, name))[0]
                for k in R.MEASURES:
                    print(f"{tag} {fault:20s} {name} {k:9s} ratio {ratio[k]:12.1f}")
                    assert ratio[k] >= 10 * bar, (tag, fault, name, k, ratio[k])
                    smallest = min(smallest, ratio[k])
    print(f"smallest planted-fault ratio {smallest:.3g}")
    assert smallest >= SMALLEST_FAULT_RATIO and all(b <= SMALLEST_FAULT_RATIO / 10 for b in R.BARS.values())


def _model():
    return detector.PointPillars(**{k: v for k, v in MODEL.items()}, test_cfg=None)


def test_modules_have_the_references_keys_and_shapes():
    g = golden("rpn")
    want = {str(k): tuple(int(d) for d in s[:n]) for k, s, n in zip(g["keys"], g["key_shapes"], g["key_ndim"])}
    assert len(want) == len(g["keys"]) > 150
    sd = _model().state_dict()
    assert set(sd) == set(want)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    neck, head = rpn.RPN(**R.NECK), rpn.CenterHead(**R.HEAD)
    assert set(neck.state_dict()) == set(R.neck_weights()) == {k[5:] for k in want if k.startswith("neck.")}
    assert set(head.state_dict()) == set(R.head_weights()) == {k[10:] for k in want if k.startswith("bbox_head.")}
    assert "blocks.0.1.weight" in R.neck_weights() and "blocks.2.16.weight" in R.neck_weights() and "deblocks.2.1.running_var" in R.neck_weights()
    assert neck.blocks[0][2].eps == 1e-3 and head.shared_conv[1].eps == 1e-5 and head.tasks[0].hm[1].eps == 1e-5
    assert float(head.tasks[0].hm[3].bias.detach()[0]) == pytest.approx(-2.19)
    assert neck.hip_serves() and head.hip_serves() and neck.downsample_factor == 1


@pytest.mark.parametrize("tag", list(R.CANVASES))
def test_composite_on_the_cpu_equals_the_recorded_fp32_outputs_bit_for_bit(tag):
    g = golden("rpn")
    neck, head = rpn.RPN(**R.NECK).eval(), rpn.CenterHead(**R.HEAD).eval()
    neck.load_state_dict({k: torch.as_tensor(v) for k, v in R.neck_weights().items()}, strict=True)
    head.load_state_dict({k: torch.as_tensor(v) for k, v in R.head_weights().items()}, strict=True)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                    # as the fixture was written
    try:
        with torch.no_grad():
            n = neck.composite(torch.from_numpy(_canvas(g, tag)))
            preds = head.composite(n)
    finally:
        torch.set_num_threads(threads)
    n = n.numpy()
    assert zlib.crc32(np.ascontiguousarray(n).tobytes()) == int(g[f"{tag}_neck_crc"])
    assert np.array_equal(n[:, ::4].view(np.uint32), g[f"{tag}_neck_f32"].view(np.uint32))
    h = R.head_cat([{k: v.numpy() for k, v in d.items()} for d in preds])
    assert list(preds[0]) == list(R.HEAD_ORDER) and np.array_equal(h.view(np.uint32), g[f"{tag}_head_f32"].view(np.uint32))


def test_unserved_configurations_run_the_composite_and_refusals():
    x = torch.rand(1, 8, 8, 12)
    gn = rpn.RPN([1], [1], [8], [1], [8], 8, norm_cfg=dict(type="GN", num_groups=2)).eval()
    assert not gn.hip_serves() and gn(x).shape == (1, 8, 8, 12)
    down = rpn.RPN([1, 1], [1, 2], [8, 8], [0.5, 1], [8, 8], 8).eval()       # a strided-convolution deblock
    assert isinstance(down.deblocks[0][0], torch.nn.Conv2d) and down.deblocks[0][0].stride == (2, 2)
    assert not down.hip_serves() and down(x).shape == (1, 16, 4, 6)
    neck = rpn.RPN(**R.NECK).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        neck(torch.zeros(1, 64, 8, 12))
    assert neck.train()(torch.rand(2, 64, 8, 12)).shape == (2, 384, 8, 12)     # train mode: the composite, anywhere
    with pytest.raises(NotImplementedError, match="dcn_head"):
        rpn.CenterHead(**dict(R.HEAD, dcn_head=True))
    with pytest.raises(NotImplementedError, match="loss is not built"):
        _model()({}, return_loss=True)
    with pytest.raises(KeyError, match="VoxelNet"):
        detector.PointPillars(**dict(MODEL, reader=dict(type="VoxelNet")))
    head = rpn.CenterHead(**R.HEAD).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head(torch.zeros(1, 384, 8, 12))
    one = rpn.SepHead(64, {"reg": (2, 2), "hm": (3, 2)}, bn=True, final_kernel=3)
    assert set(one.state_dict()) >= {"reg.0.weight", "reg.1.running_mean", "reg.3.bias", "hm.3.weight"}


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dal3.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRIES:
        assert name + "(" in header and name in hip.SIGNATURES and hasattr(lib, name), name
    assert "DAL3_CONV2D_3X3 = 0, DAL3_CONV2D_1X1 = 1, DAL3_CONV2D_DECONV2 = 2, DAL3_CONV2D_DECONV4 = 3" in header
    assert (hip.CONV2D_3X3, hip.CONV2D_1X1, hip.CONV2D_DECONV2, hip.CONV2D_DECONV4) == (0, 1, 2, 3)
    assert "Non-finite inputs and weights are" in header and "outside the contract" in header
    assert "dal3_conv2d.hip" in open(os.path.join(ROOT, "3dal_pytorch_amd", "csrc", "Makefile")).read()
    assert hip.lib().dal3_version() == 170


def test_pack_sizes_follow_the_layout():
    """the folded bias of every GEMM row padded to tiles of 32, then one float4 per lane per (out tile, 8 input channels, tap)"""
    f = hip.lib().dal3_conv2d_pack_floats
    assert f(hip.CONV2D_3X3, 64, 64) == 64 + 2 * 8 * 9 * 256
    assert f(hip.CONV2D_3X3, 64, 3) == 32 + 1 * 8 * 9 * 256
    assert f(hip.CONV2D_3X3, 20, 33) == 64 + 2 * 3 * 9 * 256
    assert f(hip.CONV2D_1X1, 64, 128) == 128 + 4 * 8 * 256
    assert f(hip.CONV2D_DECONV2, 128, 128) == 512 + 16 * 16 * 256
    assert f(hip.CONV2D_DECONV4, 256, 128) == 2048 + 64 * 32 * 256
    assert f(4, 64, 64) == 0 and f(-1, 64, 64) == 0 and f(0, 0, 64) == 0 and f(0, 64, 0) == 0 and f(0, 4097, 1) == 0


FAKE = 0x1000                                   # never dereferenced: every case fails before a launch


def _args(**kw):
    m = hip.Map(FAKE, 64 * 96, 12, 1, 96)
    a = hip.Conv2dArgs(kind=hip.CONV2D_3X3, stride=1, relu=1, c_in=64, c_out=64, y_channels=64, y_channel_offset=0,
                       max_workgroups=0, B=1, H=8, W=12, x=m, y=hip.Map(FAKE, 64 * 96, 12, 1, 96), packed=FAKE)
    for k, v in kw.items():
        if k in ("x_data", "y_data"):
            getattr(a, k[0]).data = v
        else:
            setattr(a, k, v)
    return a


def test_argument_errors_without_a_gpu():
    lib = hip.lib()
    assert lib.dal3_conv2d(None, None) == hip.EINVAL and b"null args" in lib.dal3_last_error()
    for kw, what in ((dict(x_data=None), b"null x / y"), (dict(y_data=None), b"null x / y"), (dict(packed=None), b"packed"),
                     (dict(packed=FAKE + 4), b"packed"), (dict(c_out=0), b"c_in / c_out"), (dict(c_in=0), b"c_in / c_out"),
                     (dict(c_out=4097), b"c_in / c_out"), (dict(stride=3), b"stride 3"), (dict(stride=0), b"stride 0"),
                     (dict(kind=hip.CONV2D_1X1, stride=2), b"stride 2"),
                     (dict(kind=hip.CONV2D_DECONV2, stride=3), b"stride 3"), (dict(kind=hip.CONV2D_DECONV4, stride=2), b"stride 2"),
                     (dict(kind=hip.CONV2D_DECONV2, stride=4), b"stride 4"), (dict(kind=4), b"kind 4"), (dict(kind=-1), b"kind -1"),
                     (dict(relu=2), b"relu"), (dict(max_workgroups=-1), b"max_workgroups"), (dict(B=-1), b"B / H / W"),
                     (dict(H=65536), b"B / H / W"), (dict(y_channel_offset=1), b"channels 1 .. 65 lie outside the output's 64"),
                     (dict(y_channels=63), b"outside the output's 63"), (dict(y_channel_offset=-1), b"outside"),
                     (dict(y_channels=384, y_channel_offset=321), b"channels 321 .. 385")):
        assert lib.dal3_conv2d(_args(**kw), None) == hip.EINVAL, kw
        assert what in lib.dal3_last_error(), (kw, lib.dal3_last_error())
    L = hip.Layer(FAKE, None, FAKE, FAKE, FAKE, FAKE, 64, 64)
    for args, what in (((None, 0, 1e-3, FAKE), b"null layer"), ((ctypes.byref(L), 0, 1e-3, None), b"null layer / out"),
                       ((ctypes.byref(L), 7, 1e-3, FAKE), b"kind 7"), ((ctypes.byref(L), 0, 0.0, FAKE), b"eps"),
                       ((ctypes.byref(L), 0, 1e-3, FAKE + 8), b"16-byte"),
                       ((ctypes.byref(hip.Layer(FAKE, None, FAKE, None, FAKE, FAKE, 64, 64)), 0, 1e-3, FAKE), b"all four"),
                       ((ctypes.byref(hip.Layer(None, None, None, None, None, None, 64, 64)), 0, 1e-3, FAKE), b"null weight"),
                       ((ctypes.byref(hip.Layer(FAKE, None, None, None, None, None, 64, 0)), 0, 1e-3, FAKE), b"c_in / c_out")):
        assert lib.dal3_conv2d_pack(*args, None) == hip.EINVAL, args
        assert what in lib.dal3_last_error(), lib.dal3_last_error()


def test_flop_count_of_the_benchmark_equals_the_layer_table():
    spec = importlib.util.spec_from_file_location("bench_detector", os.path.join(ROOT, "tools", "bench_detector.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    neck, head = rpn.RPN(**R.NECK), rpn.CenterHead(**R.HEAD)
    algo, executed = tool.flop(neck, head, 468, 468, 1)
    assert algo == R.table_flop(468, 468) == 447748134912              # 223.9 GMAC per 468 x 468 frame
    assert tool.flop(neck, head, 468, 468, 4)[0] == 4 * algo and executed > algo
    # by hand: four 64 -> 64 layers at 468^2, six at 234^2 (one of them 64 -> 128) and six at 117^2, the deblocks, the head
    px = 468 * 468
    hand = 9 * (4 * 64 * 64 * px + (64 * 128 + 5 * 128 * 128) * px // 4 + (128 * 256 + 5 * 256 * 256) * px // 16) \
        + 64 * 128 * px + 128 * 128 * 4 * px // 4 + 256 * 128 * 16 * px // 16 + 9 * (384 * 64 + 5 * 64 * 64 + 64 * 11) * px
    assert algo == 2 * hand
    assert len(R.layer_table(468, 468)) == 16 + 3 + 1 + 10
