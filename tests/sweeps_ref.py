"""NumPy restatement of the Waymo sweep merge (det3d/datasets/pipelines/loading.py:61-91, 140-168, the WaymoDataset branch of
LoadPointCloudFromFile) as include/dal3.h defines dal3_sweep_merge, and the door to tests/golden/sweeps.npz, which
tests/golden/gen_sweeps.py records from the reference itself.

A batch is a list of samples, a sample a list of nsweeps segments (xyz (n, 3) float32, feature (n, 2) float32,
transform_matrix (4, 4) float64 | None, time_lag), the current frame first. `merge` gives the rows
[x', y', z', tanh(feature0), feature1 (, time)] and the batch's offsets.

The arithmetic that is pinned: the transform is ((m0 x + m1 y) + m2 z) + m3 in float64, each operation rounded on its own,
cast to float32 once (the reference's `dot` is a BLAS call whose order of summation is its own: the fixture's inputs are
chosen so that every order gives the same float32, see gen_sweeps.py); tanh is the float64 tanh cast once (the reference
takes NumPy's float32 tanh, whose error the fixture records)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweeps.npz")

# intensities every segment starts with, as far as it has rows: zero, negatives, a float32 denormal, 1e5 (tanh is exactly
# 1), NaN and both infinities
SPECIAL = np.array([0.0, -0.5, -3.0, 1e-40, 1e5, np.nan, np.inf, -np.inf], np.float32)
# case -> (nsweeps, per sample the segments' (rows, matrix kind, time_lag)); matrix kinds: None, "km" (a rotation and a
# translation of kilometres), "near" (next to the identity). Rows cover 0, 1, 63, 64, 65 and 257; "two" and "three" have an
# empty sample in the middle and an empty sweep.
CASES = {
    "one": (1, [[(257, None, 0.0)]]),
    "one_b3": (1, [[(64, None, 0.0)], [(0, None, 0.0)], [(65, None, 0.0)]]),
    "two_b1": (2, [[(63, None, 0.0), (65, "km", 0.1)]]),
    "two": (2, [[(65, None, 0.0), (63, "near", 0.100021)], [(0, None, 0.0), (0, "km", 0.1)], [(257, None, 0.0), (0, "near", 0.05)],
                [(1, None, 0.0), (64, None, 0.099)]]),
    "three": (3, [[(64, None, 0.0), (1, "near", 0.1), (63, None, 0.2)], [(0, None, 0.0), (0, None, 0.1), (0, "km", 0.2)],
                  [(1, None, 0.0), (0, "km", 0.1), (257, "km", 0.199987)]]),
}


def transform(xyz, matrix):
    """rows 0 .. 2 of matrix . [x, y, z, 1] in the pinned order, float64, cast once"""
    m = np.asarray(matrix, np.float64)
    x, y, z = (xyz[:, c].astype(np.float64) for c in range(3))
    return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], 1).astype(np.float32)


def tanh32(v):
    """the float64 tanh of float32 values, cast once"""
    with np.errstate(all="ignore"):
        return np.tanh(np.asarray(v, np.float32).astype(np.float64)).astype(np.float32)


def merge(samples, nsweeps):
    """-> (points (N, 5 | 6) float32, offsets (B + 1) int64)"""
    cols = 5 if nsweeps == 1 else 6
    rows, offsets = [np.zeros((0, cols), np.float32)], [0]
    for sample in samples:
        assert len(sample) == nsweeps
        for k, (xyz, feature, matrix, time_lag) in enumerate(sample):
            xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
            feature = np.asarray(feature, np.float32).reshape(-1, 2)
            if k and matrix is not None:
                xyz = transform(xyz, matrix)
            parts = [xyz, tanh32(feature[:, :1]), feature[:, 1:]]
            if nsweeps > 1:
                parts.append(np.full((xyz.shape[0], 1), np.float32(time_lag if k else 0.0), np.float32))
            rows.append(np.concatenate(parts, 1))
        offsets.append(offsets[-1] + sum(s[0].shape[0] for s in sample))
    return np.concatenate(rows), np.asarray(offsets, np.int64)


_cache = {}


def golden():
    """the fixture, loaded once and shared (read-only)"""
    if "z" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["z"] = {k: z[k] for k in z.files}
        for v in _cache["z"].values():
            v.setflags(write=False)
    return _cache["z"]


def case(name):
    """-> (nsweeps, samples as `merge` takes them, the recorded arrays of the case: points, offsets, tanh_truth, tanh_ref_err)"""
    z = golden()
    nsweeps, layout = CASES[name]
    samples = []
    for b, segs in enumerate(layout):
        sample = []
        for k, (n, kind, time_lag) in enumerate(segs):
            key = f"{name}_s{b}_k{k}_"
            xyz, feature = z[key + "xyz"], z[key + "feature"]
            assert xyz.shape == (n, 3) and feature.shape == (n, 2)
            sample.append((xyz, feature, z[key + "matrix"] if kind else None, time_lag))
        samples.append(sample)
    want = {k: z[f"{name}_{k}"] for k in ("points", "offsets", "tanh_truth", "tanh_ref_err")}
    return nsweeps, samples, want


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                                       np.ascontiguousarray(b).view(np.uint32))


def same_bits_or_both_nan(a, b):
    """bit equality, a NaN matching any NaN: IEEE-754 leaves the payload that tanh gives a NaN to the implementation"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    eq = np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)
    return bool(np.all(eq | (np.isnan(a) & np.isnan(b))))


def tanh_error(col, feature0):
    """max |float64(col) - tanh64(feature0)| over the finite intensities"""
    f = np.asarray(feature0, np.float32).astype(np.float64)
    ok = np.isfinite(f)
    if not ok.any():
        return 0.0
    return float(np.abs(col.astype(np.float64)[ok] - np.tanh(f[ok])).max())


def feature0_of(samples):
    return np.concatenate([np.zeros(0, np.float32)] + [seg[1][:, 0] for sample in samples for seg in sample])
