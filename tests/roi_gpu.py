"""What tests/test_gpu_roi.py and tests/test_gpu_two_stage.py share: tensors on the device, the hold against roi_ref.BARS,
and the record of every figure held under DAL3_ROI_RECORD=<path> (how profiles/roi_measured.json is made: run both files
in one session)."""
import json
import os

import numpy as np
import pytest
import torch

import roi_ref as R

_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """imported by both test files: each writes all the figures held so far when its last test is done"""
    yield
    path = os.environ.get("DAL3_ROI_RECORD")
    if path and _RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _rows(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a[:, None]


def _hold(row, got, f32, truth):
    """each measure <= bar x the fp32 yardstick's own error against the truth, dead channels +0"""
    ratio, m, y = R.ratios(_rows(got), _rows(f32), _rows(truth))
    _RECORD[row] = {"measured": {k: m[k] for k in R.MEASURES}, "yardstick": {k: y[k] for k in R.MEASURES}, "ratio": ratio}
    for k in R.MEASURES:
        print(f"{row:44s} {k:9s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:7.2f}  bar {R.BARS[k]:g}")
    assert m["dead_ok"]
    bad = [(k, m[k], ratio[k]) for k in R.MEASURES if ratio[k] > R.BARS[k]]
    assert not bad, (row, bad)
