"""What the GPU tests of the PointPillars reader share (tests/test_gpu_pillars.py, tests/test_gpu_pillars_edges.py): the
upload, the voxelisation run with its standing checks, the bit-for-bit comparison, the reader module with the seeded
weights, and the judgement against the float64 truth under pillars_ref.BARS, which also keeps every figure for
DAL3_PILLARS_RECORD=<path> (how profiles/pillars_measured.json is made: run both files in one session)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import pillars_ref as R

pillars = importlib.import_module("3dal_pytorch_amd.pillars")
_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """imported by both test files: each writes all the figures held so far when its last test is done"""
    yield
    path = os.environ.get("DAL3_PILLARS_RECORD")
    if path and _RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _run(points, off, cfg, max_voxels, reverse=True, **kw):
    """-> the collated batch as host arrays, and the result object"""
    r = pillars.voxelize(_dev(points), off, cfg["voxel_size"], cfg["pc_range"], cfg["max_points"], max_voxels, reverse, **kw)
    voxels, coords, num, nv = r.finish()
    assert int(r.status.item()) == 0
    # everything behind the last voxel is zero
    m = voxels.shape[0]
    assert not r.voxels[m:].any() and not r.num_points[m:].any() and not r.coordinates[m:].any()
    return (voxels.cpu().numpy(), coords.cpu().numpy(), num.cpu().numpy(), nv.cpu().numpy()), r


def _same(got, want):
    for a, b in zip(got, want):
        assert a.shape == b.shape, (a.shape, b.shape)
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def _module(n_layers, C=5, cfg=R.PILLAR):
    net = pillars.PillarFeatureNet(num_input_features=C, num_filters=(64,) * n_layers, voxel_size=cfg["voxel_size"],
                                   pc_range=cfg["pc_range"], norm_cfg=dict(type="BN1d", eps=R.EPS, momentum=0.01))
    net.load_state_dict({k: torch.as_tensor(v) for k, v in R.reader_weights(n_layers, C).items()}, strict=True)
    return net.cuda().eval()


def _hold(row, got, f32, truth):
    ratio, m, y = R.ratios(got, f32, truth)
    _RECORD[row] = {"measured": {k: m[k] for k in R.MEASURES}, "yardstick": {k: y[k] for k in R.MEASURES}, "ratio": ratio}
    for k in R.MEASURES:
        print(f"{row:28s} {k:9s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:7.2f}  bar {R.BARS[k]:g}")
    assert m["dead_ok"]
    bad = [(k, m[k], ratio[k]) for k in R.MEASURES if ratio[k] > R.BARS[k]]
    assert not bad, (row, bad)
