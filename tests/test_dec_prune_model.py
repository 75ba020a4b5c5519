"""The per-crop pruning of dconv1 on the CPU model (tests/dec_prune_model.py): the bound, the flags and the plan's layout,
on the oracle's layers with the bench weights and crops, on planted edge cases, and the judge against planted faults."""
import importlib

import numpy as np
import pytest
import torch

import dec_prune_model as M

synth = importlib.import_module("3dal_pytorch_amd.synth")
R = importlib.import_module("oracle.ref_heads")


def _bench(n_crops, n_pts):
    sd = R.as_torch_sd(synth.state_dict("static_one"))
    pts_np, _, _ = synth.static_crops(n_crops, n_pts)
    pts = torch.from_numpy(pts_np).transpose(2, 1).contiguous()
    x2, gb, w1a = M.layers(sd, pts)
    return pts, x2, gb, w1a


@pytest.fixture(scope="module")
def bench64():
    pts, x2, gb, w1a = _bench(64, 1024)
    P, Q = M.coefficients(w1a)
    U, X = M.encoder_side(w1a, x2, pts.transpose(2, 1))
    return dict(pts=pts, x2=x2, gb=gb, w1a=w1a, P=P, Q=Q, U=U, X=X, flagged=M.flags(gb, U, X, P, Q))


def _no_flagged_channel_is_positive(w1a, gb, x2, flagged):
    for b in range(x2.shape[0]):
        rows = np.nonzero(flagged[b].numpy())[0]
        if len(rows):
            acc = M.chain_from_gb(w1a.numpy()[rows], gb[b].numpy()[rows], x2[b].numpy())
            assert not (acc > 0).any(), (b, rows[(acc > 0).any(1)])


def test_bench_crops_flag_0_43_and_never_a_live_channel(bench64):
    d = bench64
    share = float(d["flagged"].double().mean())
    print(f"flagged share on 64 bench crops: {share:.4f}")
    assert share >= 0.43
    _no_flagged_channel_is_positive(d["w1a"], d["gb"], d["x2"], d["flagged"])
    live = (~d["flagged"]).sum(1)
    print(f"live channels per crop: {int(live.min())} - {int(live.max())}, mean {float(live.double().mean()):.1f}")


def test_the_bound_holds_per_point(bench64):
    d = bench64
    E = M.bound(d["gb"][:8], d["X"][:8], d["P"], d["Q"])
    worst = M.judge_bound(d["w1a"], d["gb"][:8], d["x2"][:8], E)
    print(f"worst |s16 - (chain - gb)| / E on 8 bench crops: {worst:.3f}")


def test_planted_maximum_at_zero_one_ulp_above_and_below(bench64):
    """gb_c set so that the channel's largest chain value sits at 0 (the largest term with no positive value), one ulp of gb
    above (live: must not be flagged) and one below; none of the three may be flagged with a positive value anywhere"""
    d = bench64
    w1a, x2, P, Q = d["w1a"], d["x2"][:2], d["P"], d["Q"]
    gb = d["gb"][:2].clone()
    planted = [(0, 5), (0, 200), (1, 77), (1, 511)]
    for b, c in planted:
        # the chain started from t: search the start whose maximum is the wanted value (the maximum is monotone in the start)
        row = w1a.numpy()[c:c + 1]
        top = lambda t: float(M.chain_from_gb(row, np.array([t], np.float32), x2[b].numpy()).max())
        # "at 0": the largest start whose maximum is not positive (the maximum moves in steps of its own ulp and need not
        # land on 0 itself); its upper neighbour is the smallest start that leaves the channel live
        up1 = lambda v: np.nextafter(v, np.float32(np.inf), dtype=np.float32)
        t = np.float32(-top(np.float32(0.0)))
        for _ in range(2000):
            if top(t) <= 0:
                break
            t = np.nextafter(t, np.float32(-np.inf), dtype=np.float32)
        for _ in range(2000):
            if top(up1(t)) > 0:
                break
            t = up1(t)
        assert top(t) <= 0 < top(up1(t)) and abs(top(t)) < 1e-5, (b, c)
        for which, start in (("zero", t), ("above", np.nextafter(t, np.float32(np.inf), dtype=np.float32)),
                             ("below", np.nextafter(t, np.float32(-np.inf), dtype=np.float32))):
            g2 = gb.clone()
            g2[b, c] = float(start)
            U, X = M.encoder_side(w1a, x2, d["pts"][:2].transpose(2, 1))
            fl = M.flags(g2, U, X, P, Q)
            _no_flagged_channel_is_positive(w1a, g2, x2, fl)
            if which == "above":
                assert top(start) > 0 and not bool(fl[b, c])


def test_activation_above_the_guard_and_non_finite_coordinates_flag_nothing(bench64):
    d = bench64
    pts = d["pts"][:4].clone()
    pts[1] *= 1e4                                          # x2 beyond the fp16 guard
    pts[2, 0, 7] = float("nan")
    pts[3, 2, 0] = float("inf")
    sd = R.as_torch_sd(synth.state_dict("static_one"))
    x2, gb, w1a = M.layers(sd, pts)
    assert float(x2[1].max()) > M.F16_GUARD
    U, X = M.encoder_side(w1a, x2, pts.transpose(2, 1))
    fl = M.flags(gb, U, X, d["P"], d["Q"])
    assert bool(fl[0].any()) and not bool(fl[1:].any())
    assert bool(torch.isnan(gb[2]).all()) and bool(torch.isnan(gb[3]).all())


def test_zero_and_nan_terms(bench64):
    d = bench64
    gb = d["gb"][:1].clone()
    gb[0, 0], gb[0, 1], gb[0, 2] = 0.0, -0.0, float("nan")
    fl = M.flags(gb, d["U"][:1], d["X"][:1], d["P"], d["Q"])
    assert not bool(fl[0, 2])
    _no_flagged_channel_is_positive(d["w1a"], torch.nan_to_num(gb, nan=0.0), d["x2"][:1], fl & ~torch.isnan(gb))


@pytest.mark.parametrize("n_pts", [33, 1000])
def test_ragged_point_counts(n_pts):
    pts, x2, gb, w1a = _bench(4, n_pts)
    P, Q = M.coefficients(w1a)
    U, X = M.encoder_side(w1a, x2, pts.transpose(2, 1))
    fl = M.flags(gb, U, X, P, Q)
    assert bool(fl.any())
    _no_flagged_channel_is_positive(w1a, gb, x2, fl)


@pytest.mark.parametrize("n_live", [0, 1, 31, 32, 33, 63, 64, 65, 288, 511, 512])
def test_plan_layout_and_counts(n_live):
    rng = np.random.default_rng(n_live)
    flagged = np.ones(512, bool)
    flagged[rng.permutation(512)[:n_live]] = False
    gb_row = rng.standard_normal(512).astype(np.float32)
    lst, gbc, nch = M.plan(flagged, gb_row)
    M.judge_plan(lst, gbc, nch, flagged, gb_row)
    want = 0 if 512 - n_live < M.MIN_DEAD else {0: 2, 1: 2, 31: 2, 32: 2, 33: 2, 63: 2, 64: 2, 65: 4, 288: 10}[n_live]
    assert nch == want
    assert (gbc.reshape(16, 32)[(n_live + 31) // 32:] == -1.0).all()


def test_the_judge_rejects_planted_faults(bench64):
    d = bench64
    # 1. a bound without the |gb| term, on a crop whose term is large: the chain from gb rounds at |gb|'s ulp
    gb = d["gb"][:1] * 0 - 3.0e7
    E = M.bound(gb, d["X"][:1], d["P"], d["Q"])
    M.judge_bound(d["w1a"], gb, d["x2"][:1], E)
    with pytest.raises(AssertionError, match="bound does not hold"):
        M.judge_bound(d["w1a"], gb, d["x2"][:1], M.bound(gb, d["X"][:1], d["P"], d["Q"], gb_term=False))
    # 2. a list out of chain order, 3. a live padding entry
    flagged = d["flagged"][0].numpy()
    gb_row = d["gb"][0].numpy()
    lst, gbc, nch = M.plan(flagged, gb_row)
    M.judge_plan(lst, gbc, nch, flagged, gb_row)
    swapped = lst.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    with pytest.raises(AssertionError, match="ascending chain order"):
        M.judge_plan(swapped, gbc, nch, flagged, gb_row)
    n = int((~flagged).sum())
    assert n % 32 != 0
    live_pad = gbc.copy()
    j, pos = n // 32, n % 32
    live_pad[32 * j + M.tile_chan(pos >> 1, pos & 1)] = 1.0
    with pytest.raises(AssertionError, match="padding entry is not dead"):
        M.judge_plan(lst, live_pad, nch, flagged, gb_row)
