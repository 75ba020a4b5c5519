"""tests/f64_ref.py's measures catch what they are for — on the CPU, no marker.

A folded-BN fp32 emulation of the segmentation net (BN folded as csrc/dal3_misc.hip folds it, layers as fp32 matrix
products, dconv1's term from `g` and the max computed as the kernels do) stands in for the kernels. Unmutated it must lie
within the bars tests/test_gpu_f64_parity.py holds the kernels to; with a fault planted it must exceed every bar the fault
is aimed at by at least 10x — which is also what caps the bars (no bar above a tenth of the smallest planted ratio).
Every figure is printed before it is asserted (`pytest -s`)."""
import numpy as np
import pytest
import torch

import f64_ref as F
import f64_rows as W
from _common import synth
from test_gpu_f64_parity import BARS

B, N, SEED = 32, 256, 5
EPS = np.float32(1e-5)
FP32 = BARS["fp32"]


def _fold(sd, layer, bn):
    w = np.asarray(sd[f"ins_seg.{layer}.weight"], np.float32)[:, :, 0]
    b = np.asarray(sd[f"ins_seg.{layer}.bias"], np.float32)
    if bn is None:
        return w, b
    g, beta, mean, var = (np.asarray(sd[f"ins_seg.{bn}.{k}"], np.float32) for k in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(var + EPS)                                            # bn_scale(): fp32 throughout
    return w * s[:, None], (b - mean) * s + beta


def _relu(x):
    return np.maximum(x, np.float32(0))


def emulate(sd, pts, fault=None, arg=None):
    """pts (B, N, c) fp32 -> dict(g, logits, act1) in fp32. fault:
    "conv5_fp16"      conv5's folded weights through fp16 (the screen's score leaking out), in the channels `arg` (all if None)
    "last_point"      the crop's last point left out of the max
    "drop_k"          dconv2's input channel `arg` dropped"""
    x = pts.astype(np.float32)
    o2 = None
    for i in range(1, 6):
        w, b = _fold(sd, f"conv{i}", f"bn{i}")
        if i == 5 and fault == "conv5_fp16":
            ch = slice(None) if arg is None else arg
            w = w.copy()
            w[ch] = w[ch].astype(np.float16).astype(np.float32)
        x = _relu(x @ w.T + b)
        if i == 2:
            o2 = x
    g = (x[:, :-1] if fault == "last_point" else x).max(1)
    w, b = _fold(sd, "dconv1", "dbn1")
    gb = g @ w[:, 64:].T + b                                              # the per-crop part: W1g' g + b1'
    x = act1 = _relu(o2 @ w[:, :64].T + gb[:, None, :])
    for i in (2, 3, 4):
        w, b = _fold(sd, f"dconv{i}", f"dbn{i}")
        if i == 2 and fault == "drop_k":
            w = w.copy()
            w[:, arg] = 0
        x = _relu(x @ w.T + b)
    w, b = _fold(sd, "dconv5", None)
    return {"g": g, "logits": x @ w.T + b, "act1": act1}


@pytest.fixture(scope="module")
def base():
    pts, _, _ = synth.static_crops(B, N, seed=SEED)
    sd = synth.state_dict("static_one", seed=SEED)
    ins = (torch.from_numpy(pts).transpose(2, 1),)
    ref = F.truth("ins_seg", sd, ins)
    yard = F.yardstick("ins_seg", sd, ins, ref64=ref)
    F.check_usable(yard, ref)
    return {"pts": pts, "sd": sd, "ref": ref, "yard": F.flat(yard), "scale": np.abs(ref["g"]).max(0)}


def _ratios(base, out):
    j = F.judge(out, base["ref"])
    r = {k: v / max(base["yard"][k], F.FLOOR) for k, v in F.flat(j).items()}
    return j, r


def _show(what, r, over=None):
    print(f"\n{what}:")
    for k, v in r.items():
        tail = f"   {v / FP32[k]:9.1f} x its bar {FP32[k]:g}" if over else ""
        print(f"   {k:18s} {v:12.2f} x the yardstick{tail}")


def test_the_yardstick_is_what_the_issue_measured(base):
    """32 x 256, seed 5: the fp32 oracle against float64 is off by 4.7e-7 on g and 1.2e-6 on the logits (whole tensor)"""
    print({k: f"{v:.3g}" for k, v in base["yard"].items()})
    assert 3e-7 < base["yard"]["g.tensor"] < 7e-7 and 8e-7 < base["yard"]["logits.tensor"] < 2e-6
    dead = float((base["scale"] == 0).mean())
    live = base["scale"][base["scale"] > 0]
    print(f"g: {dead:.1%} of the channels are 0 in the truth, live maxima {live.min():.3g} .. {live.max():.3g}")
    assert 0.05 < dead < 0.5 and live.max() / live.min() > 1000


def test_the_unmutated_emulation_lies_within_the_bars(base):
    j, r = _ratios(base, emulate(base["sd"], base["pts"]))
    _show("folded-BN fp32 emulation, no fault", r)
    for k, v in r.items():
        assert v <= FP32[k], (k, v, FP32[k])
    assert j["g"]["dead_ok"]
    F.flips_legal(j["logits"], "emulation")
    assert j["g"]["tensor"] < 1e-5 and j["logits"]["tensor"] < 1e-5


AIMED = {
    "conv5_fp16": ("g.tensor", "g.chan_rms", "logits.tensor"),
    "last_point": ("g.tensor", "g.chan_rms", "g.chan_max", "logits.tensor", "logits.chan_rms", "logits.margin"),
    "drop_k": ("logits.tensor", "logits.chan_rms", "logits.margin"),
}


def _live_k(base):
    """an input channel of dconv2 whose activation is not zero on the batch: the first one live on half of the points"""
    act = emulate(base["sd"], base["pts"])["act1"]
    k = int(np.nonzero((act > 0).mean((0, 1)) > 0.5)[0][0])
    assert float(act[:, :, k].max()) > 0
    return k


@pytest.mark.parametrize("fault", list(AIMED))
def test_a_planted_fault_exceeds_every_bar_it_is_aimed_at_tenfold(base, fault):
    arg = _live_k(base) if fault == "drop_k" else None
    j, r = _ratios(base, emulate(base["sd"], base["pts"], fault, arg))
    _show(f"planted: {fault}" + (f" (k = {arg})" if arg is not None else ""), r, over=True)
    for k in AIMED[fault]:
        assert r[k] >= 10 * FP32[k], (fault, k, r[k], FP32[k])
    if fault == "drop_k":                                                 # the encoder is untouched, as it must be
        clean, _ = _ratios(base, emulate(base["sd"], base["pts"]))
        assert j["g"]["tensor"] == clean["g"]["tensor"] and j["g"]["chan_max"] == clean["g"]["chan_max"]


def test_a_dead_input_channel_changes_nothing(base):
    """why the dropped k-term must be a live one: zeroing a ReLU-dead input is invisible to every measure"""
    act = emulate(base["sd"], base["pts"])["act1"]
    dead = np.nonzero(act.max((0, 1)) == 0)[0]
    assert dead.size, "no dconv2 input is dead on the batch"
    a = emulate(base["sd"], base["pts"], "drop_k", int(dead[0]))["logits"]
    assert np.array_equal(a, emulate(base["sd"], base["pts"])["logits"])


def test_eight_small_channels_pass_the_whole_tensor_measure_and_fail_the_per_channel_ones(base):
    """the fp16-weight score used for only 8 channels of g, the live ones with the smallest scale: today's measure at
    today's bar does not see it, the per-channel measures exceed their bars tenfold"""
    live = np.nonzero(base["scale"] > 0)[0]
    small = live[np.argsort(base["scale"][live])[:8]]
    j, r = _ratios(base, emulate(base["sd"], base["pts"], "conv5_fp16", small))
    _show(f"planted: conv5 through fp16 in channels {small.tolist()} (maxima {base['scale'][small].min():.3g} .. "
          f"{base['scale'][small].max():.3g})", r, over=True)
    print(f"   g.tensor = {j['g']['tensor']:.3g}, logits.tensor = {j['logits']['tensor']:.3g} (today's bar: 1e-4)")
    assert j["g"]["tensor"] < 1e-4 and j["logits"]["tensor"] < 1e-4
    assert r["g.chan_rms"] >= 10 * FP32["g.chan_rms"], (r["g.chan_rms"], FP32["g.chan_rms"])
    assert r["g.chan_max"] >= 10 * FP32["g.chan_max"], (r["g.chan_max"], FP32["g.chan_max"])


@pytest.mark.parametrize("name", list(W.ROWS))
def test_every_rows_yardstick_is_usable(name):
    """finite measures, no live channel with a scale below 1e-30, fewer than half of g's channels zero in the truth"""
    c = W.case(name)
    F.check_usable(c["yardstick"], c["truth"])
    print(name, {k: f"{v:.3g}" for k, v in F.flat(c["yardstick"]).items()}, "dead g channels:", c["yardstick"]["g"]["n_dead"])
