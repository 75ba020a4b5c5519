"""dal3_sweep_merge behind waymo.merge_sweeps, and waymo.SweepLoader's arena, on the GPU. The expectation is
tests/golden/sweeps.npz, the reference's LoadPointCloudFromFile on the same inputs (tests/golden/gen_sweeps.py): xyz,
feature1, time, the offsets and the row order bit for bit; the tanh column bit for bit against the correctly rounded float64
truth the fixture carries (a NaN matching any NaN), so that its error against float64 is no larger than the reference's own,
which is asserted per case. The loader runs on a five-frame synthetic sequence."""
import importlib

import numpy as np
import pytest
import torch

import sweeps_ref as R

waymo = importlib.import_module("3dal_pytorch_amd.waymo")
synth = importlib.import_module("3dal_pytorch_amd.synth")
pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def _upload(samples):
    return [[(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(f)).to(DEV), m, t)
             for x, f, m, t in sample] for sample in samples]


def _check(name, got, off_dev, off_host, samples, want, nsweeps):
    ref = want["points"]
    assert got.shape == ref.shape and got.dtype == np.float32
    exact = [0, 1, 2, 4] + ([5] if nsweeps > 1 else [])
    for c in exact:
        assert R.same_bits(got[:, c], ref[:, c]), f"{name}: column {c}"
    assert np.array_equal(off_host, want["offsets"]) and np.array_equal(off_dev, want["offsets"])
    f0 = R.feature0_of(samples)
    assert R.same_bits_or_both_nan(got[:, 3], want["tanh_truth"]), f"{name}: tanh is not the correctly rounded float64 value"
    mine, theirs = R.tanh_error(got[:, 3], f0), float(want["tanh_ref_err"])
    print(f"{name}: tanh error against float64 {mine:.3e}, the reference's {theirs:.3e}")
    assert mine <= 1.0 * theirs
    assert np.all(got[f0 == np.float32(1e5), 3] == np.float32(1.0))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_recorded_case_bit_for_bit(name):
    """also: max_workgroups = 1 against the default, guard words behind the output, an output that is only 4-byte aligned
    (the narrow stores), and no synchronisation"""
    nsweeps, samples, want = R.case(name)
    dev = _upload(samples)
    n, cols = want["points"].shape
    waymo.merge_sweeps(dev, nsweeps)                          # warm: the library is loaded, the allocator has its blocks
    torch.cuda.synchronize()
    runs = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for wg, shift in ((0, 0), (1, 0), (0, 1)):
            buf = torch.full((n * cols + GUARD + shift,), float("nan"), dtype=torch.float32, device=DEV)
            buf.view(torch.int32).fill_(0x7FC0BEEF)
            off_guard = torch.full((len(samples) + 1 + 2,), -12345, dtype=torch.int64, device=DEV)
            out = buf[shift:shift + n * cols].view(n, cols)
            pts, off, off_dev = waymo.merge_sweeps(dev, nsweeps, max_workgroups=wg, out=out,
                                                   point_offsets_device=off_guard[:len(samples) + 1])
            runs.append((pts, off, off_dev, buf, off_guard, shift))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    first = None
    for pts, off, off_dev, buf, off_guard, shift in runs:
        got = pts.cpu().numpy()
        _check(name, got, off_dev.cpu().numpy(), off, samples, want, nsweeps)
        raw = buf.view(torch.int32).cpu().numpy()
        assert np.all(raw[:shift] == 0x7FC0BEEF) and np.all(raw[shift + n * cols:] == 0x7FC0BEEF), "guard words were written"
        assert off_guard[-2:].tolist() == [-12345, -12345]
        if first is None:
            first = got
        assert np.array_equal(first.view(np.uint32), got.view(np.uint32)), "max_workgroups or the alignment changes the bits"


def test_refusals():
    nsweeps, samples, _ = R.case("two_b1")
    dev = _upload(samples)
    with pytest.raises(ValueError, match="nsweeps is 3"):
        waymo.merge_sweeps(dev, 3)
    with pytest.raises(RuntimeError, match="lives on cpu"):
        waymo.merge_sweeps([[(torch.zeros(2, 3), torch.zeros(2, 2), None, 0.0)]], 1)
    with pytest.raises(ValueError, match="xyz rows"):
        waymo.merge_sweeps([[(dev[0][0][0], dev[0][1][1], None, 0.0)]], 1)
    with pytest.raises(ValueError, match="current frame"):
        waymo.merge_sweeps([[(dev[0][0][0], dev[0][0][1], np.eye(4), 0.0)]], 1)


# ---------------------------------------------------------------------------------------------- the loader
@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    """five frames of one sequence with two and with three sweeps, and what merge_sweeps gives on fresh uploads of each frame"""
    root = tmp_path_factory.mktemp("waymo")
    out = {}
    for nsweeps in (2, 3):
        info_path, infos = synth.waymo_files(str(root / f"s{nsweeps}"), 7, n_sequences=1, n_frames=5, n_points=700, nsweeps=nsweeps)
        ds = waymo.WaymoDataset(info_path, str(root), nsweeps=nsweeps)
        fresh = []
        for i in range(len(ds)):
            sample = []
            for path, matrix, lag in ds.sweeps(i):
                xyz, feature = waymo.read_frame(path)
                sample.append((xyz.to(DEV), feature.to(DEV), matrix, lag))
            pts, off, _ = waymo.merge_sweeps([sample], nsweeps)
            fresh.append(pts.cpu().numpy())
            # the restatement on the same files
            host = [(x.cpu().numpy(), f.cpu().numpy(), m, t) for x, f, m, t in sample]
            want, _ = R.merge([host], nsweeps)
            assert R.same_bits_or_both_nan(fresh[-1], want)
        out[nsweeps] = (ds, fresh)
    return out


def _run(loader):
    got, tokens = [], []
    for pts, off, off_dev, meta in loader:
        assert np.array_equal(off_dev.cpu().numpy(), off) and len(meta) == len(off) - 1
        p = pts.cpu().numpy()
        got += [p[off[b]:off[b + 1]] for b in range(len(meta))]
        tokens += [m["token"] for m in meta]
    return got, tokens


@pytest.mark.parametrize("batch_size", [1, 2])
def test_a_sequence_uploads_each_file_once(sequence, batch_size):
    ds, fresh = sequence[2]
    loader = waymo.SweepLoader(ds, batch_size, DEV)
    assert loader.capacity == batch_size + 2 and len(loader) == (5 + batch_size - 1) // batch_size
    got, tokens = _run(loader)
    assert tokens == [f"seq_0_frame_{f}.pkl" for f in range(5)]
    assert loader.uploads == 5, "frame t is sweep 0 of frame t + 1: five files, not ten"
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, fresh))
    assert got[0].shape[0] == 2 * 700 and got[1].shape[0] == 700 + 717 and got[0].shape[1] == 6


def test_a_small_arena_reads_again_and_gives_the_same_bits(sequence):
    ds, fresh = sequence[3]
    loader = waymo.SweepLoader(ds, 1, DEV, capacity=2)        # three files a frame, two kept: one comes back every step
    got, _ = _run(loader)
    assert loader.uploads > 5 and len(loader.arena) == 2
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, fresh))
    roomy = waymo.SweepLoader(ds, 1, DEV)
    got2, _ = _run(roomy)
    assert roomy.uploads == 5
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got2, fresh))


def test_the_loader_does_not_synchronise(sequence):
    ds, _ = sequence[2]
    list(waymo.SweepLoader(ds, 2, DEV))                       # warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batches = list(waymo.SweepLoader(ds, 2, DEV))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(batches) == 3 and batches[-1][1].size == 2
