"""The PointPillars reader on the GPU where the fixtures of tests/test_gpu_pillars.py (two toy grids, square in x and y,
B <= 4, two radix passes) do not reach: every pass count of the voxeliser's sort and `none` on a power of 256, keys up to bit
30, grids whose three extents differ, 300 samples with points in no sample, a run over several sort chunks with max_points
above a chunk, DAL3_PILLAR_OVERFLOW, a canvas that is not square, pillars outside it, every n_pillars, max_workgroups of
the feature kernel, and the decoration at the far corner of the production grid.

Voxelisation is compared bit for bit with pillars_ref.voxelize_batch, which tests/test_pillars_cpu.py pins to the
sequential loop (pillars_ref.voxelize_loop, itself pinned to the reference's recorded output) on these same cases. The
feature net is judged as in tests/test_gpu_pillars.py. Every input is seeded; the largest is 12000 points."""
import importlib

import numpy as np
import pytest
import torch

import pillars_ref as R
from pillars_gpu import _dev, _hold, _module, _record_file, _run, _same       # _record_file: the autouse fixture

hip = importlib.import_module("3dal_pytorch_amd._hip")
pillars = importlib.import_module("3dal_pytorch_amd.pillars")
pytestmark = pytest.mark.gpu

SENT_F, SENT_I = 0x7fc00001, -7                 # prefills: a NaN's bits for float outputs (held as int32), -7 for integers


def _want(pts, off, cfg, cap, reverse=True):
    return R.voxelize_batch(pts, off, cfg["voxel_size"], cfg["pc_range"], cfg["max_points"], cap, reverse)


def _int64(n):
    return torch.tensor([n], dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------------------------- voxelisation
@pytest.mark.parametrize("name", list(R.KEY_WIDTHS))
def test_every_pass_count_and_key_width(name):
    """1, 2, 3 and 4 passes of the sort (one pass ends in the second ping-pong buffer), `none` = B * cells on and one short
    of 2^8 and 2^16, the production grid, keys up to bit 30. On the 5 x 17 x 3 grid both coordinate layouts: each column
    reaches its own axis' last cell (4, 16, 2: x and y lie beyond the smallest extent), so no two axes can be swapped."""
    vs, rng, grid, B, none, passes = R.KEY_WIDTHS[name]
    pts, off, cfg = R.key_width_case(name)
    formed = R.sort_passes(B, R.grid_of(vs, rng))               # as launch_voxelize forms them, from the grid
    print(f"{name:10s} grid {R.grid_of(vs, rng).tolist()} B {B}  B * cells {formed[0]}  passes {formed[1]}")
    assert formed == (none, passes)
    for reverse in (True, False) if name == "2^8-1" else (True,):
        want = _want(pts, off, cfg, R.KEY_MAX_VOXELS, reverse)
        assert want[3][B - 1] > 0                               # keys above (B - 1) * cells occur
        for mw in (0, 2):
            got, r = _run(pts, off, cfg, R.KEY_MAX_VOXELS, reverse, max_workgroups=mw)
            _same(got, want)
            assert r.voxel_offsets.cpu().tolist() == np.concatenate([[0], np.cumsum(want[3])]).tolist()
        if name == "2^8-1":
            co = got[1]
            assert [int(co[:, c].max()) for c in ((3, 2, 1) if reverse else (1, 2, 3))] == [4, 16, 2]


@pytest.mark.parametrize("max_points", R.RUN_MAX_POINTS)
def test_a_run_over_several_chunks_and_max_points_above_a_chunk(max_points):
    """8998 points of one cell (a run over three sort chunks, ending at sorted entry N) and 3 of another (points 0, 4096
    and 9000; its run starts at sorted entry 0): each voxel holds its cell's first min(max_points, count) points in order;
    with max_voxels = 1 the large cell, which appears second, is dropped whole"""
    pts = R.run_length_points()
    cfg = dict(R.PILLAR, max_points=max_points)
    small = np.asarray(R.RUN_SMALL_AT)
    big = np.setdiff1d(np.arange(R.RUN_N), small)
    for cap in (2, 1):
        want = _want(pts, [0, R.RUN_N], cfg, cap)
        for mw in (0, 2):
            got, _ = _run(pts, [0, R.RUN_N], cfg, cap, max_workgroups=mw)
            _same(got, want)
            voxels, coords, num, nv = got
            assert nv.tolist() == [cap] and num.tolist() == [min(3, max_points), min(big.size, max_points)][:cap]
            assert voxels[0, :num[0], 3].tolist() == small[:max_points].tolist() and not voxels[0, num[0]:].any()
            assert coords[0].tolist() == [0, 0, R.RUN_SMALL_CELL[1], R.RUN_SMALL_CELL[0]]
            if cap == 2:
                assert np.array_equal(voxels[1, :num[1], 3], big[:max_points].astype(np.float32)) and not voxels[1, num[1]:].any()
                assert coords[1].tolist() == [0, 0, R.RUN_BIG_CELL[1], R.RUN_BIG_CELL[0]]


def test_three_hundred_samples_with_points_in_no_sample():
    """more samples than the offsets kernel has threads, a run of 211 empty ones, sizes either side of the 256-point tile,
    the cap met behind the 256th sample, and in-range points in front of offsets[0] and behind offsets[B] that must be
    dropped"""
    pts, off = R.many_samples()
    cfg = R.PILLAR
    want = _want(pts, off, cfg, R.BIG_CAP)
    nv, sizes = want[3], np.diff(off)
    for mw in (0, 2):
        got, r = _run(pts, off, cfg, R.BIG_CAP, max_workgroups=mw)
        _same(got, want)
        vo = r.voxel_offsets.cpu().numpy()
        assert np.array_equal(vo, np.concatenate([[0], np.cumsum(nv)]))
        assert not np.diff(vo)[sizes == 0].any()                # an empty sample: equal consecutive offsets
    assert (sizes == 0)[45:256].all() and nv[256:].max() == R.BIG_CAP and (nv[256:] > 0).sum() >= 5
    voxels, coords, num, _ = got
    for b in (3, 5, 7, 259, 262, 263):                          # a sample alone gives the rows it has in the batch
        alone, _ = _run(pts[off[b]:off[b + 1]], [0, int(sizes[b])], cfg, R.BIG_CAP)
        rows = coords[:, 0] == b
        assert alone[3][0] == nv[b] > 0
        _same((voxels[rows], coords[rows, 1:], num[rows]), (alone[0], alone[1][:, 1:], alone[2]))


def _raw_voxelize(pts, host_off, dev_off, cfg, max_voxels, capacity, rows, status0):
    """dal3_voxelize through the raw entry with host and device offsets of the caller's choice, on outputs of `rows`
    (>= capacity) rows prefilled with SENT_F / SENT_I -> (voxels as int32 bits, coordinates, num_points, voxel_offsets, status)"""
    p = _dev(pts)
    N, C = p.shape
    T, B = cfg["max_points"], len(host_off) - 1
    voxels = torch.full((rows, T, C), SENT_F, dtype=torch.int32, device="cuda")
    coords = torch.full((rows, 4), SENT_I, dtype=torch.int32, device="cuda")
    num = torch.full((rows,), SENT_I, dtype=torch.int32, device="cuda")
    vo = torch.full((B + 1,), SENT_I, dtype=torch.int64, device="cuda")
    status = torch.full((1,), status0, dtype=torch.int32, device="cuda")
    host, d_off = np.ascontiguousarray(host_off, np.int64), _dev(np.asarray(dev_off, np.int64))
    lib = hip.lib()
    ws = torch.empty(lib.dal3_voxelize_workspace_bytes(B, N), dtype=torch.uint8, device="cuda")
    a = hip.VoxelizeArgs(B=B, N=N, points=hip.ptr(p), point_stride=C, C=C, reverse_index=1, point_offsets=hip.ptr(d_off),
                         point_offsets_host=host.ctypes.data, max_points=T, max_voxels=max_voxels, capacity=capacity,
                         voxels=hip.ptr(voxels), coordinates=hip.ptr(coords), num_points=hip.ptr(num), voxel_offsets=hip.ptr(vo),
                         status=hip.ptr(status), max_workgroups=0, workspace=hip.ptr(ws), workspace_bytes=ws.numel())
    a.voxel_size[:], a.pc_range[:] = list(cfg["voxel_size"]), list(cfg["pc_range"])
    a.grid[:] = [int(v) for v in R.grid_of(cfg["voxel_size"], cfg["pc_range"])]
    hip.check(lib.dal3_voxelize(a, hip.stream()))
    torch.cuda.synchronize()
    return voxels, coords, num, vo, status


@pytest.mark.parametrize("status0", [0, 64])
def test_device_offsets_that_disagree_with_the_hosts(status0):
    """host offsets (0, 10, 20) give capacity 20; device offsets (0, 3000, 6000) give 50 + 50 voxels: the rows that fall
    outside the capacity set DAL3_PILLAR_OVERFLOW (OR-ed into the caller's status) and are not written. The outputs have
    2 * max_voxels rows, so every row the device offsets could name lies inside the tensors. In the other direction, device
    offsets (0, 4, 9), there is no overflow and the result is that of the device's offsets."""
    cfg, cap, capacity, rows = R.PILLAR, R.OVERFLOW_CAP, 20, 100
    pts = R.in_range_points("overflow", R.OVERFLOW_N)
    want = _want(pts, R.OVERFLOW_OFFSETS[0], cfg, cap)
    assert want[3].tolist() == [cap, cap]
    voxels, coords, num, vo, status = _raw_voxelize(pts, [0, 10, 20], R.OVERFLOW_OFFSETS[0], cfg, cap, capacity, rows, status0)
    print(f"status {int(status[0])} (prefilled {status0})  sentinel rows intact "
          f"{bool((voxels[capacity:] == SENT_F).all() and (coords[capacity:] == SENT_I).all() and (num[capacity:] == SENT_I).all())}")
    assert int(status[0]) == status0 | hip.PILLAR_OVERFLOW
    assert (voxels[capacity:] == SENT_F).all() and (coords[capacity:] == SENT_I).all() and (num[capacity:] == SENT_I).all()
    _same((voxels[:capacity].view(torch.float32).cpu().numpy(), coords[:capacity].cpu().numpy(), num[:capacity].cpu().numpy()),
          (want[0][:capacity], want[1][:capacity], want[2][:capacity]))
    result = pillars.VoxelizeResult(voxels[:capacity].view(torch.float32), coords[:capacity], num[:capacity], vo, status, 2)
    with pytest.raises(RuntimeError, match="DAL3_PILLAR_OVERFLOW"):
        result.finish()
    # fewer points on the device than the host said
    want = _want(pts, R.OVERFLOW_OFFSETS[1], cfg, cap)
    m = int(want[3].sum())
    assert 0 < m <= 9
    voxels, coords, num, vo, status = _raw_voxelize(pts, [0, 10, 20], R.OVERFLOW_OFFSETS[1], cfg, cap, capacity, rows, status0)
    assert int(status[0]) == status0
    assert vo.cpu().tolist() == np.concatenate([[0], np.cumsum(want[3])]).tolist()
    assert (voxels[capacity:] == SENT_F).all() and (coords[capacity:] == SENT_I).all() and (num[capacity:] == SENT_I).all()
    assert not voxels[m:capacity].any() and not coords[m:capacity].any() and not num[m:capacity].any()
    _same((voxels[:m].view(torch.float32).cpu().numpy(), coords[:m].cpu().numpy(), num[:m].cpu().numpy()), want[:3])


# ------------------------------------------------------------------------------------- the reader and the canvas
NX, NY, CANVAS_B, CANVAS_P = 40, 24, 3, 50
N_PILLARS = (0, 1, 49, 50, 55, -3)
OUTSIDE = {3: (-1, 5, 5), 10: (3, 5, 5), 17: (0, -1, 7), 24: (1, 24, 7), 31: (2, 9, -1), 48: (0, 9, 40)}      # row: (b, y, x)
CORNERS = {0: (0, 0, 0), 1: (1, 23, 39), 2: (2, 0, 39), 49: (0, 23, 0)}


def _canvas_pillars():
    """-> (voxels (50, 20, 5), num_points, coordinates [b, 0, y, x], inside (50) bool): 44 pillars on a 24 x 40 canvas of 3
    samples, its four corners among them, and six that lie outside it by one of b, y and x"""
    P, T, C = CANVAS_P, 20, 5
    co = np.zeros((P, 4), np.int32)
    for p in range(P):
        cell = (p * 37 + 11) % (NY * NX)
        co[p] = (p % CANVAS_B, 0, cell // NX, cell % NX)
    for p, (b, y, x) in list(OUTSIDE.items()) + list(CORNERS.items()):
        co[p] = (b, 0, y, x)
    inside = np.array([p not in OUTSIDE for p in range(P)])
    assert np.unique(co[inside][:, [0, 2, 3]], axis=0).shape[0] == inside.sum() == 44
    vox = R.synth.uniform(R.SEED, "canvas", (P, T, C), -1.0, 1.0).astype(np.float32)
    num = (1 + (np.arange(P) * 7) % T).astype(np.int32)
    vox[np.arange(T)[None, :] >= num[:, None]] = 0
    return vox, num, co, inside


@pytest.mark.parametrize("n_layers", [2, 1])
def test_a_canvas_that_is_not_square_pillars_outside_it_and_every_n_pillars(n_layers):
    """the fused store and the two-step scatter on a 24 x 40 canvas (a swapped ny / nx moves a cell), with pillars outside
    it in every direction and n_pillars 0, 1, one short of P, P, above P and negative: the canvas is the scatter of the
    first min(max(n, 0), P) pillars that lie inside it, +0 elsewhere, the same bits by both routes"""
    vox, num, co, inside = _canvas_pillars()
    P = CANVAS_P
    net = _module(n_layers)
    d = (_dev(vox), _dev(num), _dev(co))
    feats = net(*d)
    f = feats.cpu().numpy()
    assert f.shape == (P, 64) and all(f[p].any() for p in (0, 49))
    scat = pillars.PointPillarsScatter(64)

    def want(n):
        live = (np.arange(P) < min(max(n, 0), P)) & inside
        return R.scatter(f[live], co[live], CANVAS_B, NY, NX)

    full = want(P)
    for p, (b, y, x) in CORNERS.items():
        assert np.array_equal(full[b, :, y, x], f[p])
    assert not np.array_equal(want(49), full) and not want(0).any()
    for n in (None,) + N_PILLARS:
        nd = None if n is None else _int64(n)
        w = full if n is None else want(n)
        fused = net.forward_canvas(*d, CANVAS_B, [NX, NY], n_pillars=nd)
        two_step = scat(feats, d[2], CANVAS_B, [NX, NY], n_pillars=nd)
        for canvas in (fused, two_step):
            assert canvas.shape == (CANVAS_B, 64, NY, NX)
            assert np.array_equal(canvas.cpu().numpy().view(np.uint32), w.view(np.uint32)), n


def _raw_features(net, d, max_workgroups, n_pillars=None, out=None):
    vox, num, co = d
    P, T, C = vox.shape
    out = torch.empty((P, 64), dtype=torch.float32, device="cuda") if out is None else out
    a = hip.PillarFeatureArgs(P=P, n_pillars=hip.ptr(n_pillars), voxels=hip.ptr(vox), num_points=hip.ptr(num), coordinates=hip.ptr(co),
                              C=C, max_points=T, n_layers=len(net.pfn_layers), c_out=64, vx=net.vx, vy=net.vy, x_offset=net.x_offset,
                              y_offset=net.y_offset, packed=hip.ptr(net.packed()), features=hip.ptr(out), canvas=None,
                              max_workgroups=max_workgroups)
    hip.check(hip.lib().dal3_pillar_features(a, hip.stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n_layers", [2, 1])
def test_max_workgroups_and_n_pillars_of_the_feature_kernel(n_layers):
    """one and three workgroups walk 50 pillars four at a time and give the bits of the uncapped grid; with n_pillars the
    rows from n on are not written"""
    vox, num, co, _ = _canvas_pillars()
    net = _module(n_layers)
    d = (_dev(vox), _dev(num), _dev(co))
    base = net(*d).cpu().numpy().view(np.uint32)
    for mw in (0, 1, 3):
        assert np.array_equal(_raw_features(net, d, mw).cpu().numpy().view(np.uint32), base), mw
    for n in N_PILLARS:
        live = min(max(n, 0), CANVAS_P)
        out = torch.full((CANVAS_P, 64), SENT_F, dtype=torch.int32, device="cuda")
        _raw_features(net, d, 3, _int64(n), out.view(torch.float32))
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:live], base[:live]) and (got[live:] == SENT_F).all(), n


def test_mean_reader_with_n_pillars():
    """VoxelFeatureExtractorV3 with n_pillars: the first min(max(n, 0), P) rows are those of the whole call; on an output
    prefilled through the raw entry the rows from n on keep the prefill"""
    vox, num, _, _ = _canvas_pillars()
    P, T, C = vox.shape
    d_vox, d_num = _dev(vox), _dev(num)
    mean = pillars.VoxelFeatureExtractorV3(num_input_features=C)
    full = mean(d_vox, d_num).cpu().numpy()
    j = R.judge(full, R.mean_f64(vox, num))
    assert j["tensor"] < 1e-6, j                                # the sum of <= 20 floats and one division
    full = full.view(np.uint32)
    for n in N_PILLARS:
        live, nd = min(max(n, 0), P), _int64(n)
        assert np.array_equal(mean(d_vox, d_num, n_pillars=nd).cpu().numpy().view(np.uint32)[:live], full[:live]), n
        out = torch.full((P, C), SENT_F, dtype=torch.int32, device="cuda")
        hip.check(hip.lib().dal3_voxel_mean(hip.ptr(d_vox), hip.ptr(d_num), P, hip.ptr(nd), T, C, hip.ptr(out), hip.stream()))
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:live], full[:live]) and (got[live:] == SENT_F).all(), n


@pytest.mark.parametrize("n_layers", [1, 2])
def test_reader_far_from_the_origin(n_layers):
    """the production grid (0.32 m cells over +-74.88 m): pillars at x and y indices 0, 1, 233, 234, 466 and 467, where the
    offset from the pillar centre cancels 74 m against 74 m; judged against the float64 truth with the torch-CPU composite
    as the yardstick (tests/test_pillars_cpu.py holds the lane-level emulation of the kernel to the same bars)"""
    cfg = R.PRODUCTION
    vox, num, co = R.far_pillars()
    net = _module(n_layers, cfg["C"], cfg)
    out = net(_dev(vox), _dev(num), _dev(co)).cpu().numpy()
    assert out.shape == (R.FAR_P, 64)
    truth = R.reader_f64(R.reader_weights(n_layers, cfg["C"]), vox, num, co, cfg["voxel_size"], cfg["pc_range"])
    with torch.no_grad():
        f32 = net.cpu().composite(torch.from_numpy(vox), torch.from_numpy(num), torch.from_numpy(co)).numpy()
    _hold(f"far/l{n_layers}", out, f32, truth)
