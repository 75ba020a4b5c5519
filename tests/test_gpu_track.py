"""dal3_track / dal3_track_match on the GPU: the tracker against the reference's PubTracker (tests/golden/tracking.npz)
and the NumPy restatement (tests/track_ref.py) on larger seeded inputs, independence from the workgroup mapping and
the batch split, the overflow status, and the GT match against the fixture — all exact."""
import importlib

import numpy as np
import pytest
import torch

import track_ref
from _common import golden

trk = importlib.import_module("3dal_pytorch_amd.track")
SEED = 2024
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _per_frame(g):
    off = np.concatenate([[0], np.cumsum(g["out_count"])])
    return [(g["box_ids"][off[f]:off[f + 1]], g["tracking_ids"][off[f]:off[f + 1]]) for f in range(len(off) - 1)]


def _dev(ct, tr, lab, sc, fo, so):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    return dict(seq_offsets=t(so), frame_offsets=t(fo), ct=t(ct), tracking=t(tr), label=t(lab.astype(np.int32)),
                score=t(sc.astype(np.float32)))


def _same(got, want):
    assert len(got) == len(want)
    for f, ((b, t), (wb, wt)) in enumerate(zip(got, want)):
        assert np.array_equal(b, wb) and np.array_equal(t, wt), f


def test_tracker_kernel_equals_the_reference_pubtracker():
    g = golden("tracking")
    inp = trk.TrackInputs(track_ref.scene(SEED))
    res = trk.track_sequences(**inp.to(DEV), capacity=inp.capacity(3))
    _same(res.frames(), _per_frame(g))
    assert res.total() == int(g["id_count"])


@pytest.mark.parametrize("max_age,score_thresh", [(3, 0.75), (1, 0.6), (0, 0.9)])
def test_tracker_kernel_equals_the_restatement_on_large_inputs(max_age, score_thresh):
    ct, tr, lab, sc, fo, so = track_ref.big_scene(11, n_seq=300)
    want, ids = track_ref.track(ct, tr, lab, sc, fo, so, max_age=max_age, score_thresh=score_thresh)
    res = trk.track_sequences(**_dev(ct, tr, lab, sc, fo, so), max_age=max_age, score_thresh=score_thresh)
    _same(res.frames(), want)
    assert res.total() == ids
    assert np.diff(fo).max() > 500                     # one sequence's frames hold > 500 detections (and live tracks)


def test_ids_do_not_depend_on_the_workgroup_mapping_or_the_batch_split():
    ct, tr, lab, sc, fo, so = track_ref.big_scene(12, n_seq=60, big_n=200)
    d = _dev(ct, tr, lab, sc, fo, so)
    want = trk.track_sequences(**d).frames()
    for wg in (1, 7, 64):
        _same(trk.track_sequences(**d, max_workgroups=wg).frames(), want)
    cut = 23                                            # sequences [0, cut) then [cut, S): the count continues on the device
    f_cut = int(so[cut])
    a = trk.track_sequences(**_dev(ct[:fo[f_cut]], tr[:fo[f_cut]], lab[:fo[f_cut]], sc[:fo[f_cut]], fo[:f_cut + 1], so[:cut + 1]))
    b = trk.track_sequences(**_dev(ct[fo[f_cut]:], tr[fo[f_cut]:], lab[fo[f_cut]:], sc[fo[f_cut]:], fo[f_cut:] - fo[f_cut],
                                   so[cut:] - f_cut), id_base=a.id_total)
    _same(a.frames() + b.frames(), want)


def test_overflow_sets_the_status_and_raises():
    ct, tr, lab, sc, fo, so = track_ref.big_scene(13, n_seq=4, big_n=300)
    res = trk.track_sequences(**_dev(ct, tr, lab, sc, fo, so), capacity=100)
    with pytest.raises(RuntimeError, match="capacity"):
        res.frames()


def test_match_kernel_equals_the_fixture():
    g = golden("tracking")
    frames = track_ref.scene(SEED)
    inp = trk.TrackInputs(frames)
    res = trk.track_sequences(**inp.to(DEV))
    boxes = np.concatenate([trk.crops.waymo_boxes(fr["box3d"]) for fr in frames]).astype(np.float32)
    gts = [fr["gt"][:, [0, 1, 2, 3, 4, 5, -1]] for fr in frames]
    goff = np.concatenate([[0], np.cumsum([len(x) for x in gts])]).astype(np.int64)
    mf, mo = trk.match_ground_truth(res, torch.from_numpy(boxes).to(DEV), torch.from_numpy(goff).to(DEV),
                                    torch.from_numpy(np.concatenate(gts).astype(np.float32)).to(DEV))
    res.check()
    off, cnt = inp.frame_offsets, g["out_count"]
    pos = np.concatenate([np.arange(off[f], off[f] + cnt[f]) for f in range(len(cnt))]).astype(np.int64)
    assert np.array_equal(mf.cpu().numpy()[pos], g["match_frame"])
    assert np.array_equal(mo.cpu().numpy()[pos], g["match_obj"])
