"""Rotated-box IoU without a GPU: the float64 oracle (tests/iou_ref.py) against analytic answers, Monte Carlo and the
reference's own CPU IoU (tests/golden/iou_ref_pairs.npz); eval.metric_samples against the boxes the reference's
`postprocessing` builds (tests/golden/eval_metrics.npz); the C ABI's argument checks; no scratch in the kernels."""
import ctypes
import importlib
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

import iou_ref
from _common import ROOT, golden, synth

hip = importlib.import_module("3dal_pytorch_amd._hip")
ev = importlib.import_module("3dal_pytorch_amd.eval")
PI = np.pi

ANALYTIC = [                                            # (a, b, BEV IoU)
    ([0, 0, 0, 4, 2, 1.5, 0.3], [0, 0, 0, 4, 2, 1.5, 0.3], 1.0),              # identical
    ([0, 0, 0, 4, 2, 1, 0], [0, 0, 0, 2, 1, 1, 0], 0.25),                     # nested 4x2 / 2x1
    ([0, 0, 0, 2, 2, 1, 0], [1, 0, 0, 2, 2, 1, 0], 1 / 3),                    # half-shifted
    ([0, 0, 0, 2, 2, 1, 0], [2, 0, 0, 2, 2, 1, 0], 0.0),                      # edge-touching
    ([0, 0, 0, 2, 2, 1, 0], [0, 0, 0, 2, 2, 1, PI / 2], 1.0),                 # square vs itself at 90 deg
    ([0, 0, 0, 4, 1, 1, 0], [0, 0, 0, 4, 1, 1, PI / 2], 1 / 7),               # a 4x1 cross
    ([3, -2, 0, 4.8, 1.8, 1.5, 0.7], [3, -2, 0, 4.8, 1.8, 1.5, 0.7 + PI], 1.0),   # yaw + pi
    ([7, 1, 0, 4, 2, 1, 1.1], [7 + 2 * np.cos(1.1), 1 + 2 * np.sin(1.1), 0, 4, 2, 1, 1.1], 1 / 3),  # half-shifted, rotated
    ([0, 0, 0, 4, 2, 1, 0], [30, 0, 0, 4, 2, 1, 0.5], 0.0),                   # far apart
]


def test_oracle_analytic_cases():
    a = np.array([c[0] for c in ANALYTIC], float)
    b = np.array([c[1] for c in ANALYTIC], float)
    want = np.array([c[2] for c in ANALYTIC])
    bev, v3 = iou_ref.paired(a, b)
    np.testing.assert_allclose(bev, want, rtol=0, atol=1e-12)
    bev_t, _ = iou_ref.paired(b, a)                                          # symmetric
    np.testing.assert_allclose(bev_t, want, rtol=0, atol=1e-12)
    same_z = (a[:, 2] == b[:, 2]) & (a[:, 5] == b[:, 5])
    np.testing.assert_allclose(v3[same_z], bev[same_z], rtol=0, atol=1e-12)   # equal z ranges: 3D = BEV


def test_oracle_3d_is_bev_times_height_for_stacked_boxes():
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.normal(0, 20, (50, 2)), rng.normal(0, 1, (50, 1)), rng.uniform(1, 5, (50, 3)),
                        rng.uniform(-PI, PI, (50, 1))], 1)
    b = a.copy()
    b[:, 2] += rng.uniform(-1.5, 1.5, 50) * a[:, 5]                          # same footprint, shifted up or down
    b[:, 5] *= rng.uniform(0.5, 1.5, 50)
    bev, v3 = iou_ref.paired(a, b)
    np.testing.assert_allclose(bev, 1.0, atol=1e-12)
    lo = np.maximum(a[:, 2] - a[:, 5] / 2, b[:, 2] - b[:, 5] / 2)
    hi = np.minimum(a[:, 2] + a[:, 5] / 2, b[:, 2] + b[:, 5] / 2)
    zo = np.clip(hi - lo, 0, None)
    np.testing.assert_allclose(v3, zo / (a[:, 5] + b[:, 5] - zo), atol=1e-12)    # footprint cancels: z IoU
    assert (v3 == 0).any() and (v3 > 0.3).any()


def test_oracle_degenerate_and_non_finite():
    a = np.array([[0, 0, 0, 0, 2, 1, 0], [0, 0, 0, 4, 2, 1, 0], [np.nan, 0, 0, 4, 2, 1, 0], [0, 0, 0, 4, 2, 1, np.inf],
                  [0, 0, 0, -4, 2, 1, 0]], float)
    b = np.array([[0, 0, 0, 0, 2, 1, 0], [0, 0, 0, 4, 2, 0, 0], [0, 0, 0, 4, 2, 1, 0], [0, 0, 0, 4, 2, 1, 0],
                  [0, 0, 0, 4, 2, 1, 0]], float)
    bev, v3 = iou_ref.paired(a, b)
    assert bev[0] == 0 and v3[0] == 0                                       # zero area on both sides: union 0 -> 0
    assert bev[1] == 1 and v3[1] == 0                                       # flat box: BEV 1, no volume overlap
    assert np.isnan(bev[2]) and np.isnan(v3[2]) and np.isnan(bev[3]) and np.isnan(v3[3])
    assert bev[4] == 0                                                      # negative length counts as 0


@pytest.mark.parametrize("seed", range(4))
def test_oracle_agrees_with_monte_carlo(seed):
    rng = np.random.default_rng(100 + seed)
    a = np.r_[rng.normal(0, 1, 3), rng.uniform(1, 5, 3), rng.uniform(-PI, PI)]
    b = np.r_[a[:3] + rng.normal(0, 1, 3), rng.uniform(1, 5, 3), rng.uniform(-PI, PI)]
    iou = iou_ref.paired(a, b)[0][0]
    mc, se = iou_ref.monte_carlo_bev(a, b, 2_000_000, seed=seed)
    assert iou > 0 and abs(iou - mc) <= 3 * se, (iou, mc, se)


def test_oracle_against_the_reference_cpu_iou():
    """The reference's boxes_iou_bev_cpu (fp32, absolute frame, intersection points sorted by angle) and this oracle
    agree to 1e-5 on at least 98 % of the pairs. Every pair beyond that is one where the oracle is shown right: it is
    symmetric in (a, b) to 1e-9 (two different clip frames) and within 4 standard errors of a Monte Carlo estimate, or
    it is a designed case with an exact answer."""
    g = golden("iou_ref_pairs")
    a, b, nd = iou_ref.fixture_pairs()
    assert nd == int(g["n_designed"]) and abs(a.sum() + b.sum() - float(g["in_sum"])) < 1e-6, "pair generator drifted"
    ref = g["iou_bev"].astype(np.float64)
    mine = iou_ref.paired(a, b)[0]
    d = np.abs(mine - ref)
    assert np.mean(d <= 1e-5) >= 0.98, np.mean(d <= 1e-5)
    exact = {0: 1.0, 1: 0.25, 2: 1 / 3, 3: 0.0, 4: 1.0, 5: 1 / 7, 6: 1.0, 7: 1.0, 10: 0.0}
    for k, v in exact.items():                                # (the stored boxes are float32: pi / 2 is not exact)
        assert abs(mine[k] - v) < 1e-6, (k, mine[k], v)
    assert ref[7] < 0.9999                                   # the reference, identical boxes at (5000.3, -3000.7)
    bad = np.nonzero(d > 1e-5)[0]
    bad = bad[bad >= nd]
    np.testing.assert_allclose(iou_ref.paired(b[bad], a[bad])[0], mine[bad], rtol=0, atol=1e-9)
    worse = 0
    for k in bad:
        mc, se = iou_ref.monte_carlo_bev(a[k], b[k], 400_000, seed=int(k))
        assert abs(mine[k] - mc) <= 4 * se + 1e-12, (k, mine[k], ref[k], mc, se)
        worse += abs(ref[k] - mc) > 4 * se
    print(f"{len(bad)} pairs beyond 1e-5; the reference is outside 4 sigma of Monte Carlo on {worse}")


@pytest.mark.parametrize("head", ["static", "dynamic"])
def test_metric_samples_reproduce_the_reference_boxes(tmp_path, head):
    """eval.metric_samples builds the same (pred, GT) pairs, types and denominator as the reference's postprocessing
    does before it calls compute_box3d_iou (recorded in eval_metrics.npz by tests/golden/gen_iou_golden.py)."""
    g = golden("eval_metrics")
    paths, *_ = synth.segment_files(str(tmp_path), int(g["segment_seed"]), n_frames=int(g["segment_n_frames"]),
                                    n_tracks=int(g["segment_n_tracks"]))
    annos = ev.Annos(ev.reorganize_info(pickle.load(open(paths["infos"], "rb"))))
    track = pickle.load(open(paths[head], "rb"))
    if head == "static":
        track = ev.preprocessing(track, annos)
    s = ev.metric_samples(track, annos, g[f"{head}_final"], static=(head == "static"))
    assert s["n_samples"] == int(g[f"{head}_n_samples"])
    assert s["pred"].shape == g[f"{head}_pred"].shape
    np.testing.assert_allclose(s["pred"], g[f"{head}_pred"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(s["gt"], g[f"{head}_gt"], rtol=0, atol=1e-9)
    assert np.array_equal(s["types"], g[f"{head}_types"])
    np.testing.assert_allclose(iou_ref.paired(s["pred"], s["gt"])[1], g[f"{head}_iou_3d"], rtol=0, atol=1e-12)
    if head == "static":
        assert s["n_samples"] > s["pred"].shape[0]           # frames without GT are in the denominator


def test_box_iou_argument_errors_without_a_gpu():
    lib = hip.lib()
    fake = ctypes.c_void_p(0x1000)                           # never dereferenced: every call fails before a launch
    big = (1 << 24) + 1
    cases = [
        (lambda: lib.dal3_box_iou_pairwise(fake, -1, fake, 4, 0, fake, None, None), b"bad argument"),
        (lambda: lib.dal3_box_iou_pairwise(fake, 4, fake, 4, 2, fake, None, None), b"bad argument"),
        (lambda: lib.dal3_box_iou_pairwise(fake, 4, fake, 4, 0, None, None, None), b"no output"),
        (lambda: lib.dal3_box_iou_pairwise(None, 4, fake, 4, 0, fake, None, None), b"null boxes"),
        (lambda: lib.dal3_box_iou_pairwise(fake, big, fake, 4, 0, fake, None, None), b"DAL3_MAX_ITEMS"),
        (lambda: lib.dal3_box_iou_pairwise(fake, 4, fake, big, 1, None, fake, None), b"DAL3_MAX_ITEMS"),
        (lambda: lib.dal3_box_iou_paired(fake, fake, -3, 0, fake, fake, None), b"bad argument"),
        (lambda: lib.dal3_box_iou_paired(fake, fake, big, 0, fake, fake, None), b"DAL3_MAX_ITEMS"),
        (lambda: lib.dal3_box_iou_paired(fake, fake, 5, 0, None, None, None), b"no output"),
    ]
    for call, word in cases:
        assert call() == hip.EINVAL
        assert word in lib.dal3_last_error(), (word, lib.dal3_last_error())
    # nothing to do is not an error and launches nothing (no GPU needed)
    assert lib.dal3_box_iou_pairwise(None, 0, None, 7, 0, fake, None, None) == 0
    assert lib.dal3_box_iou_paired(None, None, 0, 1, fake, fake, None) == 0


def test_iou_kernels_use_no_scratch(tmp_path):
    """The clipped polygon lives in registers: .private_segment_fixed_size is 0 for every kernel of dal3_iou.hip."""
    csrc = os.path.join(ROOT, "3dal_pytorch_amd", "csrc")
    out = tmp_path / "iou.s"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
                    "--cuda-device-only", "-S", os.path.join(csrc, "dal3_iou.hip"), "-o", str(out)], check=True)
    text = out.read_text()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(kernels) == 4 and sum("pairwise" in k for k in kernels) == 2, kernels
    assert len(sizes) == len(kernels) and all(int(s) == 0 for s in sizes), sizes
