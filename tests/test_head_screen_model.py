"""The error bound, the seed rule and the candidate rule of the screened point heads on the CPU
(tests/head_screen_model.py): on bench crops and on adversarial items the fp32 arg-max of every (item, channel) is a seed
point or a candidate, a pair that is skipped can never raise the pooled value, the candidate counts are those the design
was sized from (printed with -s), and the inputs of tests/test_gpu_head_screen.py do go through the screen."""
import json

import numpy as np
import pytest
import torch

import head_screen_model as H
from _common import synth

# the design's table (DESIGN.md "Screened conv4 of the point heads"): stride -> seed share of the live tiles, candidates
# per screened tile mean / p99 / max
TABLE = {2: (0.514, 109, 670, 761), 3: (0.377, 142, 770, 916), 4: (0.268, 166, 566, 856), 6: (0.208, 229, 928, 1327),
         8: (0.148, 268, 972, 1424)}


@pytest.fixture(scope="module")
def bench():
    sd = synth.state_dict("static_one")
    obj, distinct = H.bench_objects(32, sd)
    return sd, obj, distinct


@pytest.mark.parametrize("stride", sorted(TABLE))
def test_bench_crops_reproduce_the_design_table(bench, stride):
    """bench weights, the first 32 bench crops, the oracle's mask re-centred at the mean margin: 359 distinct points per
    item on average (54 ... 512), 0.715 of the 32 x 16 tiles live, worst error 0.085 E. Weights and crops are
    deterministic, so the table's figures hold to its printed digits: the margins below are the rounding of those digits
    plus the freedom "products summed in fp32 in any order" leaves the CPU's matmul (2 % on a mean, 5 % on a tail
    quantile or a maximum, 10 % on a worst-case ratio)."""
    sd, obj, distinct = bench
    assert abs(distinct.mean() - 359) < 0.5 and distinct.min() == 54 and distinct.max() == 512
    rep = H.run(sd, obj, distinct, stride=stride, what="bench")
    print(json.dumps(rep))
    share, mean, p99, top = TABLE[stride]
    assert abs(rep["live_share"] - 0.715) < 0.0005 and abs(rep["seed_share"] - share) < 0.0005
    assert abs(rep["err_over_E"] - 0.085) < 0.0085 + 0.0005
    assert abs(rep["cand_mean"] - mean) < 0.02 * mean + 0.5
    assert abs(rep["cand_p99"] - p99) < 0.05 * p99 + 0.5 and abs(rep["cand_max"] - top) <= 0.05 * top
    assert rep["tiles_dense_for_range"] == 0
    if stride <= 4:
        assert rep["cand_max"] <= H.SCR_CAP and rep["tiles_over_cap"] == 0.0       # capacity 1024 holds the model's maximum


@pytest.mark.parametrize("scale4,shift4", [(1.0, 0.0), (1e3, 0.0), (1e-3, 0.0), (1.0, -50.0)])
def test_adversarial_items(bench, scale4, shift4):
    """duplicated points, all points equal, one live point, coordinates x 1e4 and x 1e-6; conv4 scaled by 1e3 / 1e-3; a bias
    that makes half of the maxima negative"""
    _, obj, distinct = bench
    sd = dict(synth.state_dict("static_one", seed=91))
    sd["box_est.conv4.weight"] = (np.asarray(sd["box_est.conv4.weight"]) * np.float32(scale4)).astype(np.float32)
    if shift4:
        bias = np.asarray(sd["box_est.bn4.bias"]).astype(np.float32).copy()
        bias[::2] += np.float32(shift4)
        sd["box_est.bn4.bias"] = bias
    o, d = H.adversarial(obj[:8], distinct[:8])
    for stride in (2, 4):
        rep = H.run(sd, o, d, stride=stride, what=f"adversarial x{scale4:g} {shift4:+g}")
        print(json.dumps(rep))


@pytest.mark.parametrize("kind,head,c_in,M", [("static_one", "box_est", 3, 512), ("dynamic", "point_emb", 4, 2560)])
def test_the_gpu_tests_inputs_go_through_the_screen(kind, head, c_in, M):
    """a CONDITION of tests/test_gpu_head_screen.py: on its ordinary inputs no tile leaves the screen for range and at
    most 1 % of the screened tiles exceed the list's capacity — the GPU tests cannot pass by running the dense fall-back
    everywhere"""
    B = H.gpu_batch(M)
    sd, x, d = H.gpu_case(kind, head, c_in, B, M)
    dense, scr, over = H.occupancy(sd, torch.from_numpy(x), d, p=head)
    print(f"{head} {B}x{M}: {scr} screened tiles, {dense} dense for range, {over} over the capacity")
    assert scr > 0 and dense == 0 and over <= 0.01 * scr
