"""The compacted body of the fp32 throughput decoder has ONE route (csrc/dal3_pointmlp.hip, DESIGN.md "Compacted
dconv2"): a fully live chunk of 32 dconv1 channels goes through the LDS slab as 16 compact k-steps in the dense order,
like every other chunk of that body, and the logits keep the dense decoder's BITS.

The harness is tests/test_gpu_dec_sparse.py's: one large launch (the throughput kernels) against the same crops in chunks
of at most 512 tiles through the latency family, every row, no tolerance. The dconv1 bias recipe is that of
`tools/ab_kernels.py --dead-frac`: +1e6 makes a channel live in every point, -1e6 dead in every point, so the crop's term
`gb` has exactly as many negative entries as there are dead channels. Every setup keeps 192 of them, which is at or above
DAL3_DEC_MIN_DEAD, so its tiles take the compacted body."""
import numpy as np
import pytest
import torch

from _common import build_model, synth
from test_gpu_dec_sparse import _blob, _check, _guard_flag, _with_dconv1_bias

pytestmark = pytest.mark.gpu

FULL = (0, 1, 3, 4, 6, 7, 9, 11, 12, 14)                    # ten whole chunks live; 2, 5, 8, 10, 13, 15 are the other six


def _ten_full_chunks():
    """+1e6 on exactly ten whole chunks of 32 channels, -1e6 on the 192 channels of the other six (scattered between
    the live chunks): 192 negative entries in `gb`, the compacted body, ten of its sixteen chunks fully live"""
    shift = np.full(512, -1e6)
    for c in FULL:
        shift[32 * c:32 * c + 32] = 1e6
    assert int((shift < 0).sum()) == 192
    return shift


def _run(shift, B, N, seed, what):
    model = build_model("static_one", _with_dconv1_bias(seed, shift))
    assert _guard_flag(_blob(model)) == 0
    pts_np, _, _ = synth.static_crops(B, N, seed=seed)
    lg, mk = _check(model, torch.from_numpy(pts_np).cuda(), 3, what)
    assert bool(torch.isfinite(lg).all())
    return lg, mk


def test_fully_live_chunks_inside_the_compacted_body():
    """runs of two fully live chunks, single ones, dead chunks between them and at the end: the slab carries every one"""
    _run(_ten_full_chunks(), 80, 1024, 71, "ten full chunks")


def test_a_fully_live_chunk_with_a_pending_channel():
    """a fully live chunk behind a chunk with an odd live count: the waiting channel is the low half of the full chunk's
    first k-step and the full chunk's last channel waits in turn (33 terms, 16 steps). The crop keeps its 192 negative
    entries (live channels outside ten full chunks would take it below them), so chunk 14 gives up its place among the
    ten: nine chunks are fully live and 32 live channels are spread with odd counts (7, 9, 5) over chunks 2, 5 and 8, each in front of a run of full chunks
    (the one after chunk 8 with the dead chunk 10 inside: the channel waits through it), and 11 in chunk 14, where the
    last waiting channel finds its partner; the total, 320, is even."""
    rng = np.random.default_rng(72)
    shift = np.full(512, -1e6)
    for c in FULL:
        if c != 14:
            shift[32 * c:32 * c + 32] = 1e6
    for c, n in ((2, 7), (5, 9), (8, 5), (14, 11)):
        shift[32 * c + rng.permutation(32)[:n]] = 1e6
    assert int((shift < 0).sum()) == 192
    _run(shift, 80, 1024, 72, "full chunk behind a waiting channel")


def test_ragged_n():
    """N = 1000: the crop's last wave replicates its last point, the fourth wave of the last workgroup has no tile"""
    _run(_ten_full_chunks(), 140, 1000, 73, "ten full chunks, ragged")
