"""tests/sweeps_ref.py, the NumPy restatement of the Waymo sweep merge, against tests/golden/sweeps.npz, the reference's own
LoadPointCloudFromFile on the same inputs (tests/golden/gen_sweeps.py): bit for bit on xyz, feature1 and time, and on the
tanh column within the reference's own recorded error against float64. Also the host half of 3dal_pytorch_amd/waymo.py:
the segment table's layout. No GPU."""
import importlib

import numpy as np
import pytest

import sweeps_ref as R


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_equals_the_recorded_reference(name):
    nsweeps, samples, want = R.case(name)
    got, offsets = R.merge(samples, nsweeps)
    ref = want["points"]
    assert got.shape == ref.shape and ref.shape[1] == (5 if nsweeps == 1 else 6)
    exact = [0, 1, 2, 4] + ([5] if nsweeps > 1 else [])
    assert R.same_bits(got[:, exact], ref[:, exact])
    assert np.array_equal(offsets, want["offsets"]) and offsets[-1] == ref.shape[0]
    # tanh: the restatement is the correctly rounded column, so its error is the floor; the reference's is the bar
    f0 = R.feature0_of(samples)
    assert R.same_bits_or_both_nan(got[:, 3], want["tanh_truth"])
    mine, theirs = R.tanh_error(got[:, 3], f0), float(want["tanh_ref_err"])
    print(f"{name}: tanh error {mine:.3e}, the reference's {theirs:.3e}")
    assert mine <= theirs and R.tanh_error(ref[:, 3], f0) == theirs
    # NaN and the infinities where the intensities have them, 1e5 -> exactly 1
    assert np.array_equal(np.isnan(got[:, 3]), np.isnan(f0))
    assert np.all(got[f0 == np.float32(1e5), 3] == np.float32(1.0)) and np.all(got[np.isneginf(f0), 3] == np.float32(-1.0))


def test_the_cases_cover_what_they_claim():
    sizes = {n for _, layout in R.CASES.values() for segs in layout for n, _, _ in segs}
    assert {0, 1, 63, 64, 65, 257} <= sizes
    assert {ns for ns, _ in R.CASES.values()} == {1, 2, 3}
    kinds = {kind for _, layout in R.CASES.values() for segs in layout for k, (_, kind, _) in enumerate(segs) if k}
    assert kinds == {None, "km", "near"}
    z = R.golden()
    # every segment still starts with the special intensities, as far as it has rows, transformed segments included
    specials = 0
    for name, (_, layout) in R.CASES.items():
        for b, segs in enumerate(layout):
            for k, (n, kind, _) in enumerate(segs):
                head = z[f"{name}_s{b}_k{k}_feature"][:R.SPECIAL.size, 0]
                assert R.same_bits(head, R.SPECIAL[:n]), (name, b, k)
                specials += int(k > 0 and kind is not None and n >= R.SPECIAL.size)
    assert specials >= 3, "NaN, the infinities, 1e5 and the denormal also ride through transformed segments"
    assert sum(v.shape[0] for k, v in z.items() if k.endswith("_points")) < 5000
    km = z["three_s2_k2_matrix"]
    assert abs(km[0, 3]) > 1000 and abs(z["two_s0_k1_matrix"] - np.eye(4)).max() < 0.5


def test_segment_record_is_the_ctypes_mirror():
    hip = importlib.import_module("3dal_pytorch_amd._hip")
    waymo = importlib.import_module("3dal_pytorch_amd.waymo")
    for name, ctype in hip.SweepSegment._fields_:
        field = getattr(hip.SweepSegment, name)
        assert waymo.SEGMENT.fields[name][1] == field.offset and waymo.SEGMENT.fields[name][0].itemsize == field.size, name
    assert waymo.SEGMENT.itemsize == 136
