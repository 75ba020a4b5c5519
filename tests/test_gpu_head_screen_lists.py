"""The candidate list of the screened fp32 point heads (csrc/dal3_screen.h in csrc/dal3_head_screen.hip: hit words parked
per block, the list built once per tile by a prefix scan, staged weight rows in the recompute) leaves the dense head's
BITS, with the harness of tests/test_gpu_head_screen.py (the per-tile dense launch, every row).

Every coordinate appears 4 times in a row under distinct indices (all counted as distinct points): the copies are
registers 4q..4q+3 of one lane half of one tile and tie in every channel, so a lane holds several hits of one block.
512 items x 512 points are 8192 tiles, the dispatch minimum of the screened route; 517 items do not divide into the
workgroups' runs."""
import numpy as np
import pytest
import torch

from _common import synth
from test_gpu_head_screen import _check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", [512, 517])
def test_points_repeated_four_times_under_distinct_indices(B):
    M = 512
    pts = synth.static_crops(B, M // 4, seed=41)[0]
    x = np.ascontiguousarray(np.repeat(pts[:, :, :3], 4, axis=1)).astype(np.float32)
    assert x.shape == (B, M, 3)
    d = np.full(B, M, np.int32)
    d[1::5] = M - 30                                       # ragged: the last tile's tail repeats the last distinct point
    f = _check("static_one", "box_est", synth.state_dict("static_one", seed=23), x, d, f"4 copies {B}x{M}")
    assert bool(torch.isfinite(f).all()) and float(f.max()) > 0
