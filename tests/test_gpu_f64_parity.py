"""The fp32 heads (and the f16x3 kernels, whose contract is "fp32 accuracy") against the float64 truth, per element.

Every row (tests/f64_rows.py) runs the kernels through the C ABI, compares with `f64_ref.truth` and asserts each measure of
`f64_ref.errors` <= bar x the fp32 oracle's own figure on the same rows (`f64_ref.yardstick`): the rule of
tests/test_gpu_lowprec.py for the 16-bit kernels against emu16, here with float64 as the truth and torch-CPU's fp32 as the
model of fp32 arithmetic. The existing TOL = 1e-4 tests stay as they are; this file is the tight judge beside them.

With DAL3_F64_RECORD=<path> in the environment the run also writes every measure, the yardstick's absolute value and their
ratio per row to <path> (how profiles/f64_parity_measured.json was made)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import f64_ref as F
import f64_rows as W
from _common import build_model

hip = importlib.import_module("3dal_pytorch_amd._hip")
pytestmark = pytest.mark.gpu

# The bars: multiples of the yardstick. Each is the worst ratio recorded in profiles/f64_parity_measured.json over the rows
# of its precision x 2, rounded up to one significant digit (at most 2x headroom over a measured worst case), and
#   * no bar exceeds a tenth of the smallest ratio a planted fault of tests/test_f64_ref_cpu.py produces for its measure
#     (asserted there: every planted fault exceeds 10 x the bar),
#   * `tensor` against float64 stays below TENSOR_ABS on every fp32 row whatever the yardstick says.
# box_pred_one (the two-stage model's first estimator) shares box_pred's bars. The per-channel measures of `g` are maxima
# (chan_rms is carried by its largest entries too) over channels whose own maximum is up to 10^4 below the layer's: an entry
# of a channel of scale 0.0026 that is off by one ulp of its partial sums (1.2e-6) reads 4.7e-4 there, and the fp32 oracle's
# own figure on such a row moves by 6x with the thread count of its convolution. That is the row (latency family, c_in 4,
# 2 x 5120) that sets their two bars; the fp32 emulation of tests/test_f64_ref_cpu.py reads 1.1x the yardstick on it.
BARS = {
    "fp32": {
        "g.tensor": 3.0, "g.chan_rms": 9.0, "g.chan_max": 20.0,
        "logits.tensor": 4.0, "logits.chan_rms": 4.0, "logits.chan_max": 4.0, "logits.margin": 4.0,
        "box_pred.tensor": 3.0, "box_pred.chan_rms": 2.0, "box_pred.chan_max": 3.0,
        "boxes7.tensor": 3.0, "boxes7.chan_rms": 2.0, "boxes7.chan_max": 3.0,
    },
    "f16x3": {
        "g.tensor": 3.0, "g.chan_rms": 4.0, "g.chan_max": 5.0,
        "logits.tensor": 4.0, "logits.chan_rms": 4.0, "logits.chan_max": 4.0, "logits.margin": 4.0,
        "box_pred.tensor": 2.0, "box_pred.chan_rms": 3.0, "box_pred.chan_max": 3.0,
        "boxes7.tensor": 2.0, "boxes7.chan_rms": 3.0, "boxes7.chan_max": 3.0,
    },
}
TENSOR_ABS = 1e-5                                          # ten times tighter than TOL, against 1e-6 claimed
_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    path = os.environ.get("DAL3_F64_RECORD")
    if path and _RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


def bar_of(precision, measure):
    return BARS[precision][measure.replace("box_pred_one.", "box_pred.")]


def hold(row, precision, got, ref, yard):
    """judge `got` against `ref`, print and record every figure, then assert the bars, +0 in the dead channels and that
    every mask flip is legal"""
    j = F.judge(got, ref)
    y = F.flat(yard)
    m = F.flat(j)
    ratio = {k: v / max(y[k], F.FLOOR) for k, v in m.items()}
    _RECORD[f"{row}/{precision}"] = {"measured": m, "yardstick": {k: y[k] for k in m}, "ratio": ratio,
                                     "flips": int(j["logits"]["flips"].size) if "logits" in j else 0}
    for k in m:
        print(f"{row:24s} {precision:6s} {k:22s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:7.2f}  bar {bar_of(precision, k):g}")
    bad = [(k, m[k], ratio[k]) for k in m if ratio[k] > bar_of(precision, k)]
    assert not bad, (row, precision, bad)
    if precision == "fp32":
        for k in m:
            if k.endswith(".tensor"):
                assert m[k] < TENSOR_ABS, (row, k, m[k])
    for k, e in j.items():
        assert e["dead_ok"], (row, k, "a channel that is 0 in the truth is not +0")
    if "logits" in j:
        F.flips_legal(j["logits"], row)
    return j


def _ins_seg(model, pts, dt=hip.F32):
    """tests/test_gpu_parity.py's _ins_seg with the precision as an argument"""
    lib = hip.lib()
    B, c_in, N = pts.shape
    w = model._cache.get("ins_seg", model.ins_seg, hip.HEAD_INS_SEG, dt)
    ws = torch.empty(lib.dal3_ins_seg_workspace_bytes(B), dtype=torch.uint8, device="cuda")
    logits = torch.empty((B, N, 2), device="cuda")
    mask = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    g = torch.empty((B, 1024), device="cuda")
    hip.check(lib.dal3_ins_seg_forward(hip.ptr(w), dt, c_in, hip.bcn(pts), B, N, hip.ptr(logits), hip.ptr(mask),
                                       hip.ptr(g), hip.ptr(ws), ws.numel(), hip.stream()))
    return logits.cpu().numpy(), mask.cpu().numpy().astype(bool), g.cpu().numpy()


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _cat(c, bp):
    return np.concatenate([c.cpu().numpy(), bp.cpu().numpy()[:, 3:]], 1)


def run_row(name, precision="fp32"):
    """the kernels' outputs on the row's whole batch, cut to the rows that are judged"""
    assert hip.DISPATCH_FLAGS == 0
    c = W.case(name)
    kind, rows = c["kind"], c["rows"]
    model = build_model("static_one" if kind == "ins_seg" else kind, c["sd"])
    pts = _dev(c["arrays"][0]).transpose(2, 1)
    logits, mask, g = _ins_seg(model, pts, hip.DTYPES[precision])
    assert np.array_equal(mask, logits[:, :, 0] < logits[:, :, 1])
    got = {"logits": logits[rows], "g": g[rows]}
    if kind == "ins_seg":
        return got
    model.precision = precision
    choice, override = torch.from_numpy(c["choice"]), torch.from_numpy(c["mask"])
    if kind == "dynamic":
        o = model._run(pts, _dev(c["arrays"][1]).transpose(2, 1), init_box8=_dev(c["arrays"][2]), choice=choice,
                       mask_override=override)
        got["box_pred"] = o["bp"].cpu().numpy()
    else:
        o = model._run(pts, _dev(c["arrays"][1]), _dev(c["arrays"][2]), choice=choice, mask_override=override)
        if kind == "static_two":
            got["box_pred_one"], got["box_pred"] = _cat(o["c1"], o["bp1"]), _cat(o["c2"], o["bp2"])
        else:
            got["box_pred"] = _cat(o["c1"], o["bp1"])
    assert np.array_equal(o["obj_idx"].cpu().numpy(), c["forced"][0].numpy()), "the teacher-forced draws did not arrive"
    assert np.array_equal(o["logits"].cpu().numpy().view(np.int32), logits.view(np.int32))
    got["boxes7"] = o["boxes7"].cpu().numpy()
    return got


@pytest.mark.parametrize("name", list(W.ROWS))
def test_fp32_row_against_float64(name):
    c = W.case(name)
    hold(name, "fp32", run_row(name), c["truth"], c["yardstick"])


@pytest.mark.parametrize("name", W.F16X3_ROWS)
def test_f16x3_row_against_float64(name):
    c = W.case(name)
    hold(name, "f16x3", run_row(name, "f16x3"), c["truth"], c["yardstick"])


def test_compacted_and_dense_decoder_rows_take_their_bodies():
    """the route of the two decoder rows, as tests/test_gpu_dec_sparse.py establishes it — no guard flag in the blob, the
    throughput family — and counted on the crop's term itself: `gb` from dal3_ins_seg_global_bias is negative in at least
    DAL3_DEC_MIN_DEAD channels of every crop of the compacted row and in none of the dense row"""
    from test_gpu_dec_sparse import _blob, _guard_flag
    lib = hip.lib()
    for name, want in (("dec_compacted_96x1024", True), ("dec_dense_96x1024", False)):
        c = W.case(name)
        model = build_model("static_one", c["sd"])
        w = _blob(model)
        assert _guard_flag(w) == 0
        pts = _dev(c["arrays"][0]).transpose(2, 1)
        B, _, N = pts.shape
        g = torch.zeros((B, 1024), device="cuda")
        gb = torch.empty((B, 512), device="cuda")
        hip.check(lib.dal3_ins_seg_encode(hip.ptr(w), hip.F32, 3, hip.bcn(pts), B, N, hip.ptr(g), hip.stream()))
        hip.check(lib.dal3_ins_seg_global_bias(hip.ptr(w), hip.F32, hip.ptr(g), B, hip.ptr(gb), hip.stream()))
        neg = (gb < 0).sum(1).cpu().numpy()
        assert (neg >= W.DEC_MIN_DEAD).all() if want else (neg == 0).all(), (name, neg.min(), neg.max())


def test_standalone_encode_global_bias_decode():
    """dal3_ins_seg_encode -> _global_bias -> _decode as separate launches. The encoder's `g` is judged as it comes; the
    decoder is fed the float64 `g` rounded to fp32, so its logits carry no encoder error in their input"""
    lib = hip.lib()
    c = W.case(W.STANDALONE_ROW)
    model = build_model("static_one", c["sd"])
    w = model._cache.get("ins_seg", model.ins_seg, hip.HEAD_INS_SEG)
    pts = _dev(c["arrays"][0]).transpose(2, 1)
    B, c_in, N = pts.shape
    g = torch.zeros((B, 1024), device="cuda")
    hip.check(lib.dal3_ins_seg_encode(hip.ptr(w), hip.F32, c_in, hip.bcn(pts), B, N, hip.ptr(g), hip.stream()))
    g64 = _dev(c["truth"]["g"].astype(np.float32))
    gb = torch.empty((B, 512), device="cuda")
    hip.check(lib.dal3_ins_seg_global_bias(hip.ptr(w), hip.F32, hip.ptr(g64), B, hip.ptr(gb), hip.stream()))
    logits = torch.empty((B, N, 2), device="cuda")
    mask = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    hip.check(lib.dal3_ins_seg_decode(hip.ptr(w), hip.F32, c_in, hip.bcn(pts), B, N, hip.ptr(gb), hip.ptr(logits),
                                      hip.ptr(mask), hip.stream()))
    lg = logits.cpu().numpy()
    assert np.array_equal(mask.cpu().numpy().astype(bool), lg[:, :, 0] < lg[:, :, 1])
    hold("standalone_16x256", "fp32", {"g": g.cpu().numpy(), "logits": lg}, c["truth"], c["yardstick"])
