"""The references of the pillar reader's training step, on the CPU (tests/pillars_train_ref.py): the truth against the
reference's recorded run (tests/golden/pillars_train.npz), the yardstick's own error, the planted faults, and the
condition on the inputs of every GPU case of tests/test_gpu_pillars_train.py."""
import numpy as np
import pytest
import torch

import pillars_ref as R
import pillars_train_ref as T

# the smallest planted-fault ratio, recorded: running_var_biased moves running_var by 766 times the yardstick's own error
# (the others by 7e5 .. 2e7); every bar has to stay under a tenth of it
SMALLEST_FAULT = 766.0


def _close(got, want, rtol):
    for row in want:
        assert got[row].shape == want[row].shape, row
        assert np.allclose(got[row], want[row], rtol=rtol, atol=rtol * np.abs(want[row]).max()), (row, np.abs(got[row] - want[row]).max())


@pytest.mark.parametrize("n_layers", (1, 2))
def test_truth_equals_the_reference_record(n_layers):
    vox, num, co, cot, rows = T.golden_inputs()
    g = np.load(T.GOLDEN + "/pillars_train.npz")
    assert np.array_equal(g["rows"], rows)
    want = T.golden_record(n_layers, "f64")
    assert set(want) == set(T.flat(T.manual(R.reader_weights(n_layers, 5), vox, num, co, cot)))
    _close(T.flat(T.composite_run(T.module(n_layers, 5), vox, num, co, cot, torch.float64)), want, 1e-11)
    _close(T.flat(T.manual(R.reader_weights(n_layers, 5), vox, num, co, cot)), want, 1e-11)
    # and the yardstick is the reference's own fp32 run up to fp32 rounding
    _close(T.flat(T.composite_run(T.module(n_layers, 5), vox, num, co, cot, torch.float32)), T.golden_record(n_layers, "f32"), 1e-4)


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_definition_and_yardstick(name):
    """the NumPy definition equals the autograd truth; the fp32 yardstick's own error is finite and non-zero on every row"""
    sd, vox, num, co, cot, _ = T.case(name)
    truth, f32 = T.references(name)
    _close(T.flat(T.manual(sd, vox, num, co, cot)), truth, 1e-11)
    for row in truth:
        y = R.judge(f32[row], truth[row])
        assert all(np.isfinite(y[k]) and y[k] > 0 for k in R.MEASURES), (row, y)


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_inputs_keep_the_margins(name):
    """no ReLU pre-activation within MARGIN of the layer's rms, no runner-up within MARGIN of its maximum: a condition on
    the inputs, found by the search in pillars_train_ref.case"""
    sd, vox, num, co, _, salt = T.case(name)
    gate, gap = T.margins(sd, vox, num, co)
    print(f"{name}: salt {salt}, gate {gate:.3e}, gap {gap:.3e}")
    assert gate > T.MARGIN and gap > T.MARGIN
    assert num[0] == 1 and num[1] == vox.shape[1]           # a pillar of 1 point and one of exactly max_points


def test_golden_inputs_keep_the_margins():
    vox, num, co, _, _ = T.golden_inputs()
    for n_layers in (1, 2):
        assert min(T.margins(R.reader_weights(n_layers, 5), vox, num, co)) > T.MARGIN


def test_planted_faults_show():
    worst = {f: T.planted(f) for f in T.FAULTS}
    for f, r in worst.items():
        print(f"{f:32s} {r:10.3g}")
    smallest = min(worst.values())
    assert smallest >= 10 * max(T.BARS.values()), worst
    assert 0.5 * SMALLEST_FAULT <= smallest <= 2 * SMALLEST_FAULT, smallest     # the recorded figure still describes it


def test_no_fault_is_no_fault():
    sd, vox, num, co, cot, _ = T.case(T.FAULT_CASE)
    truth, f32 = T.references(T.FAULT_CASE)
    got = T.flat(T.manual(sd, vox, num, co, cot))
    assert max(max(r[0].values()) for r in T.ratios(got, f32, truth).values()) < 1e-3


def test_slice_constant_is_mirrored():
    assert T.SLICE == 128 and {c[3] for c in T.CASES.values()} >= {T.SLICE - 1, T.SLICE, T.SLICE + 1, 2 * T.SLICE + 3}
