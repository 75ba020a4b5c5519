"""The error bound and the candidate rules of the screened encoder on the CPU (tests/screen_model.py): on bench crops and
on adversarial ones the candidate set always holds the fp32 arg-max, a pair that is skipped can never raise the pooled
value, and the candidate counts are those the design was sized from (printed with -s)."""
import json

import numpy as np
import pytest
import torch

import screen_model as S
from _common import synth
from oracle import ref_heads as R


def _case(sd, pts_np, what):
    x4, w5, b5 = S.activations(R.as_torch_sd(sd), torch.from_numpy(pts_np).transpose(2, 1))
    rep = S.check(w5, b5, x4, what)
    print(json.dumps({k: v for k, v in rep.items() if not k.startswith("_")}))
    return rep


def test_bench_crops_reproduce_the_design_table():
    """bench weights, the 32 bench crops of the design's table (per-pair bounds): l2 1.82 mean / 13 max candidates per
    (crop, channel), worst error 0.15 eps; l1 1.33 / 8, 0.31 eps. Weights and crops are deterministic, so the table's
    figures hold to its printed digits: the margins below are the rounding of those digits (0.005) plus the freedom
    "products summed in fp32 in any order" leaves the CPU's matmul (2 % on a mean, 10 % on a worst-case ratio).
    The kernels' per-wave bound on the same 32 crops: 2.66 (the diagnostic build counts 2.60 on the MI355X over all 4096
    crops, of which these are the first 32, with thresholds that other workgroups have already raised in flight). No
    32-point tile comes near the list's capacity (the fall-back's cap: at most 1 % of tiles)."""
    rep = _case(synth.state_dict("static_one"), synth.static_crops(32, 1024)[0], "bench")
    assert abs(rep["l2"]["cand_mean"] - 1.82) < 0.04 and rep["l2"]["cand_max"] <= 13 and abs(rep["l2"]["err_over_eps"] - 0.15) < 0.02
    assert abs(rep["l1"]["cand_mean"] - 1.33) < 0.03 and rep["l1"]["cand_max"] <= 8 and abs(rep["l1"]["err_over_eps"] - 0.31) < 0.035
    k = rep["kernel"]
    assert 1.8 < k["cand_mean"] < 2.9 and k["tiles_over_cap"] <= 0.01 and k["per_tile_max"] <= S.SCR_CAP // 2
    assert k["dense_points"] == 0.0


def _adversarial(pts_np):
    p = pts_np.copy()
    N = p.shape[1]
    p[0, N // 2:] = p[0, :N // 2]                          # duplicated points: exact ties
    p[1, :] = p[1, 0]                                       # all points equal
    p[2] *= np.float32(1e4)                                 # coordinates of 1e4
    p[3] *= np.float32(1e-6)                                # ... and of 1e-6
    p[4, 200:264] *= np.float32(300.0)
    p[5, :] = 0.0
    return p


@pytest.mark.parametrize("scale5,shift5", [(1.0, 0.0), (1e3, 0.0), (1e-3, 0.0), (1.0, -50.0)])
def test_adversarial_crops(scale5, shift5):
    """ties, constant crops, huge and tiny coordinates, conv5 scaled by 1e3 / 1e-3, channels whose maximum is negative"""
    sd = dict(synth.state_dict("static_one", seed=91))
    sd["ins_seg.conv5.weight"] = (np.asarray(sd["ins_seg.conv5.weight"]) * np.float32(scale5)).astype(np.float32)
    if shift5:
        bias = np.asarray(sd["ins_seg.bn5.bias"]).astype(np.float32).copy()
        bias[::2] += np.float32(shift5)
        sd["ins_seg.bn5.bias"] = bias
    rep = _case(sd, _adversarial(synth.static_crops(8, 1024, seed=91)[0]), f"adversarial x{scale5:g} {shift5:+g}")
    if shift5:
        # a channel whose maximum is negative pools to +0: none of its points may be a candidate (without the rule
        # "an upper bound <= 0 cannot raise g" every point of the crop would be one)
        cand, top = rep["_cand"][:, ::2], rep["_top"][:, ::2]
        # s16 + E + b <= chain + 2 E + b <= top + 2 emax: where that is negative the upper bound of every pair is, too
        gone = top + 2.0 * rep["_emax"][:, ::2] < 0
        assert float(gone.double().mean()) > 0.8 and int(cand[gone].max()) == 0
