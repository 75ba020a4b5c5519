#!/usr/bin/env python3
"""Generate tests/golden/sweeps.npz from the REAL reference (jacky121298/3DAL_PyTorch): `LoadPointCloudFromFile` with
dataset="WaymoDataset" (det3d/datasets/pipelines/loading.py:61-91, 140-168) on tests/sweeps_ref.py's CASES, the frame files
written to a temporary directory in the converter's format.

Run only where the reference checkout exists (DAL3_REFERENCE, default /root/reference):
    python tests/golden/gen_sweeps.py

loading.py is loaded by path behind stub modules, as gen_nms.py loads its files: it imports pycocotools, det3d.torchie and
det3d.core.box_np_ops, none of which the Waymo branch touches.

The condition on the inputs, which makes bit equality a fair demand of any implementation whatever its order of summation:
the reference's transform is a float64 BLAS `dot` of a 4 x 4 matrix with [x, y, z, 1], rounded to float32 when it is
assigned back. Every transformed coordinate is evaluated here EXACTLY (Python fractions of the float64 matrix entries and
the float32 coordinates), and a point is drawn again
  - if the exact value lies within 8 float64 ulps of a float32 rounding boundary, an ulp being that of the largest of the
    four terms and the result (a float64 sum of four terms in any order, fused or not, stays well inside that), or
  - if the float32 the reference recorded is not the correctly rounded exact value.
The same for the intensity: the truth is the float64 `np.tanh` of the float32 value, and a value is drawn again if that
truth moved by 4 ulps either way rounds to another float32 (sweeps_ref.SPECIAL's values pass, which is asserted). Recorded
with each case: the correctly rounded tanh column, and the reference's own float32 error against the float64 truth
(max |float64(reference) - tanh64| over the finite intensities), the bar the implementations are held to.
"""
import math
import os
import pickle
import sys
import tempfile
import types
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gen_nms  # noqa: E402
import sweeps_ref as R  # noqa: E402

RNG = np.random.RandomState(20251)


def import_loading():
    registry = types.SimpleNamespace(register_module=lambda cls: cls)
    gen_nms._stub("pycocotools", mask=gen_nms._stub("pycocotools.mask"))
    gen_nms._stub("det3d", torchie=gen_nms._stub("det3d.torchie"))
    gen_nms._stub("det3d.core", box_np_ops=gen_nms._stub("det3d.core.box_np_ops"))
    for name in ("det3d.datasets", "det3d.datasets.pipelines"):
        gen_nms._stub(name)
    gen_nms._stub("det3d.datasets.registry", PIPELINES=registry)
    return gen_nms._load_file("det3d.datasets.pipelines.loading", "det3d/datasets/pipelines/loading.py")


def matrix_of(kind):
    yaw, t = (0.7853, [1234.567, -2345.678, 12.3]) if kind == "km" else (1e-4, [0.35, -0.02, 0.001])
    yaw += RNG.uniform(-1e-3, 1e-3) if kind == "km" else RNG.uniform(-1e-5, 1e-5)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    m[:3, 3] = np.asarray(t) + RNG.uniform(-0.5, 0.5, 3) * (1.0 if kind == "km" else 1e-3)
    return m


def draw_xyz(n):
    return (RNG.uniform(-1.0, 1.0, (n, 3)) * [75.0, 75.0, 3.0]).astype(np.float32)


def draw_intensity(n):
    return (RNG.uniform(0.0, 1.0, n) ** 3 * 4.0).astype(np.float32)


def exact_ok(matrix, xyz, got):
    """per point: every transformed coordinate clear of the float32 rounding boundaries and `got` correctly rounded"""
    ok = np.ones(xyz.shape[0], bool)
    for i, p in enumerate(xyz):
        for r in range(3):
            terms = [Fraction(float(matrix[r, c])) * Fraction(float(p[c])) for c in range(3)] + [Fraction(float(matrix[r, 3]))]
            exact = sum(terms)
            f32 = np.float32(float(exact))
            big = max([abs(t) for t in terms] + [abs(exact)])
            margin = 8 * Fraction(math.ulp(float(big)))
            lo = (Fraction(float(np.nextafter(f32, np.float32(-np.inf)))) + Fraction(float(f32))) / 2
            hi = (Fraction(float(np.nextafter(f32, np.float32(np.inf)))) + Fraction(float(f32))) / 2
            if not (np.isfinite(f32) and lo + margin < exact < hi - margin and got[i, r].tobytes() == f32.tobytes()):
                ok[i] = False
    return ok


def tanh_ok(v):
    """-> (per value: the float64 truth +- 4 ulps rounds to one float32, that float32)"""
    with np.errstate(all="ignore"):
        t = np.tanh(v.astype(np.float64))
        truth = t.astype(np.float32)
        lo, hi = (t - 4 * np.spacing(np.abs(t))).astype(np.float32), (t + 4 * np.spacing(np.abs(t))).astype(np.float32)
    return ~np.isfinite(t) | ((lo == truth) & (hi == truth)), truth


def run_reference(loading, tmp, name, nsweeps, samples):
    """the reference on one batch, a sample at a time as its data set calls it -> the collated rows"""
    load = loading.LoadPointCloudFromFile(dataset="WaymoDataset")
    rows = []
    for b, sample in enumerate(samples):
        paths = []
        for k, (xyz, feature, _, _) in enumerate(sample):
            paths.append(os.path.join(tmp, f"{name}_{b}_{k}.pkl"))
            with open(paths[-1], "wb") as f:
                pickle.dump({"lidars": {"points_xyz": xyz.copy(), "points_feature": feature.copy()}}, f)
        info = {"path": paths[0], "sweeps": [{"path": p, "transform_matrix": s[2], "time_lag": s[3]}
                                             for p, s in zip(paths[1:], sample[1:])]}
        with np.errstate(all="ignore"):
            res, _ = load({"lidar": {"nsweeps": nsweeps}}, info)
        rows.append(res["lidar"]["combined"] if nsweeps > 1 else res["lidar"]["points"])
    out = np.concatenate(rows)
    assert out.dtype == np.float32
    return out


def main():
    loading = import_loading()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (nsweeps, layout) in R.CASES.items():
            samples = []
            for segs in layout:
                sample = []
                for n, kind, time_lag in segs:
                    feature = np.stack([draw_intensity(n), RNG.uniform(-1.0, 2.0, n).astype(np.float32)], 1).reshape(n, 2)
                    feature[:min(n, R.SPECIAL.size), 0] = R.SPECIAL[:n]
                    sample.append([draw_xyz(n), feature, matrix_of(kind) if kind else None, time_lag])
                samples.append(sample)
            for attempt in range(50):
                got = run_reference(loading, tmp, name, nsweeps, samples)
                redrawn, row = 0, 0
                for sample in samples:
                    for k, seg in enumerate(sample):
                        xyz, feature, matrix, _ = seg
                        n = xyz.shape[0]
                        part = got[row:row + n]
                        row += n
                        # each column is drawn again on its own margin: a point that fails only the xyz margin keeps its
                        # intensity, so a special value is never replaced
                        bad_t = ~tanh_ok(feature[:, 0])[0]
                        assert not bad_t[:R.SPECIAL.size].any(), "a special intensity fails the tanh margin"
                        bad_x = np.zeros(n, bool)
                        if k and matrix is not None:
                            bad_x = ~exact_ok(matrix, xyz, part[:, :3])
                        else:
                            assert R.same_bits(part[:, :3], xyz)
                        if bad_x.any():
                            xyz[bad_x] = draw_xyz(int(bad_x.sum()))
                        if bad_t.any():
                            feature[bad_t, 0] = draw_intensity(int(bad_t.sum()))
                        redrawn += int(bad_x.sum()) + int(bad_t.sum())
                if not redrawn:
                    break
                print(f"{name}: attempt {attempt}: {redrawn} points drawn again")
            else:
                raise RuntimeError(f"{name}: the margins were not met in 50 attempts")
            mine, offsets = R.merge(samples, nsweeps)
            f0 = R.feature0_of(samples)
            truth = tanh_ok(f0)[1]
            exact = [0, 1, 2, 4] + ([5] if nsweeps > 1 else [])
            assert R.same_bits(mine[:, exact], got[:, exact]), name
            assert R.same_bits_or_both_nan(mine[:, 3], truth), name
            ref_err = R.tanh_error(got[:, 3], f0)
            assert R.tanh_error(mine[:, 3], f0) <= ref_err, name
            for b, sample in enumerate(samples):
                for k, (xyz, feature, matrix, _) in enumerate(sample):
                    assert R.same_bits(feature[:R.SPECIAL.size, 0], R.SPECIAL[:xyz.shape[0]]), "the special intensities are recorded"
                    key = f"{name}_s{b}_k{k}_"
                    out[key + "xyz"], out[key + "feature"] = xyz, feature
                    if matrix is not None:
                        out[key + "matrix"] = matrix
            out[f"{name}_points"], out[f"{name}_offsets"] = got, offsets
            out[f"{name}_tanh_truth"], out[f"{name}_tanh_ref_err"] = truth, np.float64(ref_err)
            ulp = R.tanh_error(got[:, 3], f0) / 2.0 ** -24
            print(f"{name}: {got.shape[0]} rows x {got.shape[1]}, reference tanh error {ref_err:.3e} ({ulp:.2f} of 2^-24), "
                  f"restatement {R.tanh_error(mine[:, 3], f0):.3e}")
    path = os.path.join(HERE, "sweeps.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
