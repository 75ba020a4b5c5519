"""The float64 judge of the fp32 heads: the oracle's own functions run on float64 tensors as the truth, per-channel
error measures beside today's whole-tensor one, and the fp32 oracle's own error on those measures as the yardstick that
every GPU bar is a multiple of (the rule tests/test_gpu_lowprec.py uses for the 16-bit kernels against emu16).

Why: `_common.rel_err` is max|a - b| / max|b| over the whole tensor against an fp32 reference. The live channels of the
pooled feature `g` span a factor of 4000 in their own maxima, so an error of 30 % of the smallest live channel passes a
1e-4 bar on that measure; and an fp32 reference is itself 5e-7 .. 1e-6 away from the exact value.

No GPU, no product code: numpy + torch-CPU + oracle/ref_heads.py only."""
import contextlib
from unittest import mock

import numpy as np
import torch

from _common import BOX7_GROUPS, BOX_PRED_GROUPS
from oracle import ref_heads as R

# A correctly rounded fp32 value is up to 2^-24 of its own magnitude away from the exact one, so a measure normalised by
# max|ref| cannot be held below that by any fp32 arithmetic; where the fp32 oracle happens to land closer than this (few
# entries, exact sums), the bar is taken on this floor instead of on a number that is zero by luck.
FLOOR = 2.0 ** -24
KINDS = ("ins_seg", "static_one", "static_two", "dynamic")


@contextlib.contextmanager
def _float64_everywhere():
    """the oracle's forwards create a few tensors at the default dtype and call `.float()` on the gathered points; with
    the default at float64 and `.float()` mapped to `.double()` they run in float64 from the first layer to the decode"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with mock.patch.object(torch.Tensor, "float", lambda self, *a, **k: self.double()):
            yield
    finally:
        torch.set_default_dtype(old)


def _cast(v, dtype):
    t = torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v.detach().cpu()
    return t.to(dtype) if t.is_floating_point() else t


def _np64(t):
    return np.asarray(t.detach().numpy() if torch.is_tensor(t) else t, np.float64)


def _box_pred(out, centre):
    """the 39 columns in `_common.BOX_PRED_GROUPS` order, the centre columns holding the head's centre output"""
    b = out["heading_scores"].shape[0]
    return np.concatenate([_np64(out[centre]), _np64(out["heading_scores"]), _np64(out["heading_residuals_normalized"]),
                           _np64(out["size_scores"]), _np64(out["size_residuals_normalized"]).reshape(b, 9)], 1)


def run(kind, sd, inputs, forced=None, dtype=torch.float64):
    """The oracle at `dtype` -> dict of float64 numpy arrays.

    kind / inputs:  "ins_seg" (pts,) | "static_one" (pts, init_box) | "static_two" (pts, init_box, bbox_gt) |
                    "dynamic" (pts, box, init_box8); pts is the logical (B, c_in, N) tensor.
    forced:         (indices (B, M) int64, counts (B,)) — the oracle's teacher forcing of the sampled points; required
                    for everything but "ins_seg" (a free-running float64 run would draw from its own mask).
    returns:        logits (B,N,2), g (B,1024); for the full models box_pred (B,39) (two-stage: box_pred_one and
                    box_pred, the second stage's) and boxes7 (B,7)."""
    assert kind in KINDS, kind
    ctx = _float64_everywhere() if dtype == torch.float64 else contextlib.nullcontext()
    with ctx, torch.no_grad():
        tsd = {k: _cast(v, dtype) for k, v in sd.items()}
        ins = [_cast(x, dtype) for x in inputs]
        logits, g = R.ins_seg(tsd, ins[0], want_global=True)
        res = {"logits": _np64(logits), "g": _np64(g)}
        if kind == "ins_seg":
            return res
        assert forced is not None, "the full models are judged teacher-forced"
        if kind == "static_one":
            out = R.static_one_forward(tsd, ins[0], ins[1], forced=forced)
            res["box_pred"] = _box_pred(out, "center")
            res["boxes7"] = _np64(R.decode_static(out, ins[1], False))
        elif kind == "static_two":
            out = R.static_two_forward(tsd, ins[0], ins[1], ins[2], forced=forced)
            one = {k[:-4]: v for k, v in out.items() if k.endswith("_one")}
            res["box_pred_one"] = _box_pred(one, "center")
            two = {k[:-4]: v for k, v in out.items() if k.endswith("_two") and k != "_object_pts_two"}
            res["box_pred"] = _box_pred(two, "center")
            res["boxes7"] = _np64(R.decode_static(out, ins[1], True))
        else:
            out = R.dynamic_forward(tsd, ins[0], ins[1], forced=forced)
            res["box_pred"] = _box_pred(out, "center")
            res["boxes7"] = _np64(R.decode_dynamic(out, ins[2]))
        assert np.array_equal(_np64(out["logits"]), res["logits"])
        return res


def truth(kind, sd, inputs, forced=None):
    """the float64 truth: every state-dict tensor and input cast to float64, the oracle's functions as they are"""
    return run(kind, sd, inputs, forced, torch.float64)


def errors(got, ref64, groups=None, logits=False):
    """Measures of `got` against the float64 `ref64` (same shape, channels on the last axis):

    tensor    max|got - ref| / max|ref| — `_common.rel_err` against float64; per column group (a tuple of (lo, hi)) for
              box tensors, the largest of the groups' own figures
    chan_rms, chan_max   |got - ref| divided by the channel's own max|ref| over the batch; rms / max over all entries of
              the channels whose scale is not zero
    dead_ok   every channel whose reference is exactly 0 everywhere holds +0 bit for bit (n_dead, n_chan beside it)
    min_scale the smallest non-zero channel scale
    margin, flips (logits=True)   max |(l1 - l0)_got - (l1 - l0)_ref| / max|ref|, and for every point whose mask
              (l0 < l1) differs from the reference's the reference's |l1 - l0| / max|ref| (a float64 array)"""
    ref = np.asarray(ref64, np.float64)
    got32 = np.asarray(got)
    got = got32.astype(np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    c = ref.shape[-1]
    d = np.abs(got - ref).reshape(-1, c)
    r = np.abs(ref).reshape(-1, c)
    spans = groups or ((0, c),)
    out = {"tensor": max(float(d[:, lo:hi].max() / max(r[:, lo:hi].max(), 1e-300)) for lo, hi in spans)}
    scale = r.max(0)
    live = scale > 0
    rel = d[:, live] / scale[live]
    out["chan_rms"] = float(np.sqrt(np.mean(rel ** 2))) if live.any() else 0.0
    out["chan_max"] = float(rel.max()) if live.any() else 0.0
    g2 = got32.reshape(-1, c)[:, ~live]
    if g2.dtype == np.float32:
        out["dead_ok"] = bool((g2.view(np.uint32) == 0).all())
    else:
        out["dead_ok"] = bool(((g2 == 0) & ~np.signbit(g2)).all())
    out["n_dead"], out["n_chan"] = int((~live).sum()), int(c)
    out["min_scale"] = float(scale[live].min()) if live.any() else 0.0
    if logits:
        top = max(float(r.max()), 1e-300)
        mg, mr = got[..., 1] - got[..., 0], ref[..., 1] - ref[..., 0]
        out["margin"] = float(np.abs(mg - mr).max() / top)
        out["flips"] = np.abs(mr[(mg > 0) != (mr > 0)]) / top
    return out


GROUPS = {"box_pred": BOX_PRED_GROUPS, "box_pred_one": BOX_PRED_GROUPS, "boxes7": BOX7_GROUPS}
SCALARS = ("tensor", "chan_rms", "chan_max", "margin")


def judge(got, ref64):
    """errors() of every tensor `got` and `ref64` share -> {name: errors dict}"""
    return {k: errors(got[k], ref64[k], GROUPS.get(k), logits=(k == "logits")) for k in ref64 if k in got}


def flat(judged):
    """{"g.tensor": .., "logits.margin": ..} — the scalar measures of judge()'s result"""
    return {f"{k}.{m}": float(e[m]) for k, e in judged.items() for m in SCALARS if m in e}


def yardstick(kind, sd, inputs, forced=None, ref64=None):
    """the same measures for the fp32 oracle — the reference as it ships — against truth()"""
    ref64 = truth(kind, sd, inputs, forced) if ref64 is None else ref64
    got = run(kind, sd, inputs, forced, torch.float32)
    got = {k: v.astype(np.float32) if k != "boxes7" else v for k, v in got.items()}
    return judge(got, ref64)


def check_usable(judged_yardstick, ref64):
    """the conditions under which a multiple of the yardstick means something (asserted on the CPU for every row)"""
    for name, v in flat(judged_yardstick).items():
        assert np.isfinite(v), (name, v)
    for k, e in judged_yardstick.items():
        assert e["min_scale"] >= 1e-30, (k, e["min_scale"])
    gz = judged_yardstick["g"]
    assert gz["n_dead"] < 0.5 * gz["n_chan"], ("g channels that are zero in the truth", gz["n_dead"])
    assert np.isfinite(ref64["logits"]).all()


def flips_legal(e_logits, what=""):
    """a mask bit may differ from the float64 mask only where the truth is within the arithmetic's own error of the
    tie: every flip's float64 |margin| / max|ref| lies below 2 x the case's measured margin error"""
    f = e_logits["flips"]
    assert f.size == 0 or float(f.max()) < 2 * e_logits["margin"], (what, f.size, float(f.max()), e_logits["margin"])
