"""CPU-side checks of the PointPillars reader (3dal_pytorch_amd/pillars.py; dal3_voxelize, dal3_pillar_features,
dal3_pillar_scatter, dal3_voxel_mean): the sort-based NumPy restatement of tests/pillars_ref.py against what the reference's
own points_to_voxel recorded (tests/golden/pillars.npz, written by tests/golden/gen_pillars.py) — which pins that the parallel
formulation equals the sequential loop, cap included —, the float64 restatement of the feature net against the reference
module's .double() output, the planted faults against the GPU test's bars, the C ABI's entries, workspace sizes and
argument checks, and the refusals that need no device. No GPU compute here."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import pillars_ref as R
from _common import ROOT, golden

hip = importlib.import_module("3dal_pytorch_amd._hip")
pillars = importlib.import_module("3dal_pytorch_amd.pillars")

ENTRIES = ("dal3_voxelize_workspace_bytes", "dal3_voxelize", "dal3_pillar_pack", "dal3_pillar_features", "dal3_pillar_scatter",
           "dal3_voxel_mean")


def _cloud(g, name):
    """(points, cfg, max_voxels, reverse) of a single-sample fixture case, checked against the fixture's checksum"""
    if name in R.PILLAR_CAPS:
        pts, cfg, cap, rev, key = R.cloud(f"pillar{int(g['pillar_salt'])}", 20000, R.PILLAR, R.PILLAR["C"]), R.PILLAR, \
            R.PILLAR_CAPS[name], True, "pillar_sum"
    else:
        C, rev = R.VOXELNET_CASES[name]
        pts, cfg, cap, key = R.cloud(f"vn{C}", 6000, R.VOXELNET, C), R.VOXELNET, R.VOXELNET["max_voxels"], name + "_sum"
    s = float(np.nan_to_num(pts.astype(np.float64), nan=3.0, posinf=5.0, neginf=7.0).sum())
    assert abs(s - float(g[key])) < 1e-9, "the seeded cloud drifted from the fixture"
    return pts, cfg, cap, rev


@pytest.mark.parametrize("name", sorted(R.PILLAR_CAPS) + sorted(R.VOXELNET_CASES))
def test_sorted_restatement_equals_the_references_loop(name):
    g = golden("pillars")
    pts, cfg, cap, rev = _cloud(g, name)
    assert np.isnan(pts[:, :3]).any() and np.isinf(pts[:, :3]).any()
    voxels, coords, num = R.voxelize(pts, cfg["voxel_size"], cfg["pc_range"], cfg["max_points"], cap, rev)
    assert np.array_equal(voxels.view(np.uint32), R.gather(pts, g[name + "_index"]).view(np.uint32))
    assert np.array_equal(coords, g[name + "_coords"]) and np.array_equal(num, g[name + "_num"])
    assert coords.dtype == np.int32 and num.dtype == np.int32
    if name == "cap600":
        assert num.size == 600 and (num == cfg["max_points"]).any()


def test_sorted_restatement_equals_the_reference_on_the_ragged_batch():
    g = golden("pillars")
    pts, off = R.batch_points()
    voxels, coords, num, nv = R.voxelize_batch(pts, off, R.PILLAR["voxel_size"], R.PILLAR["pc_range"], R.PILLAR["max_points"],
                                               R.BATCH_CAP)
    assert nv.tolist() == g["batch_num_voxels"].tolist() and nv[1] == 0 and nv[2] == 0 and nv[0] == R.BATCH_CAP
    assert np.array_equal(voxels.view(np.uint32), R.gather(pts, g["batch_index"]).view(np.uint32))
    assert np.array_equal(coords, g["batch_coords"]) and np.array_equal(num, g["batch_num"])


def _index_equals_loop(pts, cfg, max_points, cap):
    """the sort-based restatement against the sequential loop on one sample -> the triple"""
    a = R.voxelize_index(pts, cfg["voxel_size"], cfg["pc_range"], max_points, cap)
    b = R.voxelize_loop(pts, cfg["voxel_size"], cfg["pc_range"], max_points, cap)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x, y)
    return b


@pytest.mark.parametrize("name", sorted(R.PILLAR_CAPS) + sorted(R.VOXELNET_CASES))
def test_sequential_loop_equals_the_references_recorded_output(name):
    """voxelize_loop is the definition of include/dal3.h written as the loop it is stated as: it reproduces what the
    reference's points_to_voxel recorded, cap1 and the NaN points included, and so anchors the new cases"""
    g = golden("pillars")
    pts, cfg, cap, rev = _cloud(g, name)
    index, cell, count = R.voxelize_loop(pts, cfg["voxel_size"], cfg["pc_range"], cfg["max_points"], cap)
    assert np.array_equal(index, g[name + "_index"]) and np.array_equal(count, g[name + "_num"])
    assert np.array_equal(cell[:, ::-1] if rev else cell, g[name + "_coords"])
    _index_equals_loop(pts, cfg, cfg["max_points"], cap)


def test_sequential_loop_equals_the_reference_on_the_ragged_batch():
    g = golden("pillars")
    pts, off = R.batch_points()
    index, coords, num = [], [], []
    for b in range(len(off) - 1):
        i, c, n = R.voxelize_loop(pts[off[b]:off[b + 1]], R.PILLAR["voxel_size"], R.PILLAR["pc_range"], R.PILLAR["max_points"],
                                  R.BATCH_CAP)
        index.append(np.where(i >= 0, i + off[b], -1))
        coords.append(np.concatenate([np.full((c.shape[0], 1), b, np.int64), c[:, ::-1]], 1))
        num.append(n)
    assert [n.size for n in num] == g["batch_num_voxels"].tolist()
    # the fixture stores the rows as points, so compare the points the indices name
    assert np.array_equal(R.gather(pts, np.concatenate(index)).view(np.uint32), R.gather(pts, g["batch_index"]).view(np.uint32))
    assert np.array_equal(np.concatenate(coords), g["batch_coords"]) and np.array_equal(np.concatenate(num), g["batch_num"])


@pytest.mark.parametrize("name", list(R.KEY_WIDTHS))
def test_key_width_cases_are_what_the_table_says_and_equal_the_loop(name):
    """grid, B * cells and the sort's passes of every row; every sample equals the sequential loop; keys reach the top of
    the row's range (the last sample holds in-range points: for `top` that is bit 30 of the key)"""
    vs, rng, grid, B, none, passes = R.KEY_WIDTHS[name]
    pts, off, cfg = R.key_width_case(name)
    assert R.grid_of(vs, rng).tolist() == list(grid) and off.size == B + 1
    assert R.sort_passes(B, R.grid_of(vs, rng)) == (none, passes)
    cells = int(np.prod(grid))
    for b in range(B):
        part = pts[off[b]:off[b + 1]]
        index, cell, count = _index_equals_loop(part, cfg, R.KEY_MAX_POINTS, R.KEY_MAX_VOXELS)
        assert 0 < count.size <= min(cells, R.KEY_MAX_VOXELS)
        if cells <= 256:
            assert count.size >= 0.95 * cells                       # the small grids fill (nearly) every cell
        key = b * cells + (cell[:, 2] * grid[1] + cell[:, 1]) * grid[0] + cell[:, 0]
        assert key.max() < none < 2 ** 31 - 1
        if b == B - 1:
            assert key.max() >= (B - 1) * cells and int(key.max()).bit_length() == (none - 1).bit_length()
    if name == "top":
        assert key.max() >> 30 == 1
    if name == "2^8-1":                                             # every axis reaches its own, different, extent
        assert cell.max(0).tolist() == [4, 16, 2]


def test_run_length_and_many_sample_cases_equal_the_loop():
    pts = R.run_length_points()
    for max_points in R.RUN_MAX_POINTS:
        index, cell, count = _index_equals_loop(pts, R.PILLAR, max_points, 2)
        small, big = np.asarray(R.RUN_SMALL_AT), np.setdiff1d(np.arange(R.RUN_N), R.RUN_SMALL_AT)
        assert count.tolist() == [min(3, max_points), min(big.size, max_points)]
        assert index[0, :count[0]].tolist() == small[:max_points].tolist()
        assert index[1, :count[1]].tolist() == big[:max_points].tolist() and (index[1, count[1]:] == -1).all()
        assert cell.tolist() == [list(R.RUN_SMALL_CELL) + [0], list(R.RUN_BIG_CELL) + [0]]
        index, cell, count = _index_equals_loop(pts, R.PILLAR, max_points, 1)       # the large cell is dropped whole
        assert count.tolist() == [min(3, max_points)] and index[0, :count[0]].tolist() == small[:max_points].tolist()
    pts, off = R.many_samples()
    sizes = np.diff(off)
    assert off.size == R.BIG_B + 1 and off[0] == R.BIG_HEAD and off[-1] == R.BIG_N - R.BIG_TAIL
    assert sizes[:9].tolist() == list(R.BIG_SIZES) and not sizes[45:256].any() and sizes[256:].max() == 257
    assert R.cells(pts[:off[0]], R.PILLAR["voxel_size"], R.PILLAR["pc_range"])[0].all()
    assert R.cells(pts[off[-1]:], R.PILLAR["voxel_size"], R.PILLAR["pc_range"])[0].all()
    capped = 0
    for b in np.nonzero(sizes)[0]:
        count = _index_equals_loop(pts[off[b]:off[b + 1]], R.PILLAR, R.PILLAR["max_points"], R.BIG_CAP)[2]
        capped += count.size == R.BIG_CAP
    assert capped >= 10                                             # the cap is met, behind the 256th sample too
    assert _index_equals_loop(pts[off[262]:off[263]], R.PILLAR, R.PILLAR["max_points"], R.BIG_CAP)[2].size == R.BIG_CAP
    # the overflow case: both sets of device offsets
    pts = R.in_range_points("overflow", R.OVERFLOW_N)
    assert R.cells(pts, R.PILLAR["voxel_size"], R.PILLAR["pc_range"])[0].all()
    for off, sizes in zip(R.OVERFLOW_OFFSETS, ([R.OVERFLOW_CAP] * 2, [4, 5])):
        got = [_index_equals_loop(pts[off[b]:off[b + 1]], R.PILLAR, R.PILLAR["max_points"], R.OVERFLOW_CAP)[2].size for b in range(2)]
        assert got == sizes


def test_faces_follow_the_definition():
    """a lower face is in, an upper face is out, one ulp either side falls as the float32 division says"""
    cfg = R.PILLAR
    pl = R.planted(cfg, 5, True)
    ok, c = R.cells(pl, cfg["voxel_size"], cfg["pc_range"])
    lo, hi = np.float32(cfg["pc_range"][0]), np.float32(cfg["pc_range"][3])
    x = pl[:9, 0]                               # below / on / above: the lower x face, the upper one, an interior one
    assert ok[:9].tolist() == [False, True, True, True, False, False, True, True, True]
    assert x[1] == lo and x[4] == hi and c[6, 0] == 2 and c[7, 0] == 3 and c[8, 0] == 3
    assert not ok[-9:].any()                    # +Inf, -Inf, NaN


def _reader_case(g, n_layers):
    pts, off = R.batch_points()
    rows = g["reader_rows"]
    return (R.reader_weights(n_layers, R.PILLAR["C"]), R.gather(pts, g["batch_index"])[rows], g["batch_num"][rows],
            g["batch_coords"][rows])


@pytest.mark.parametrize("n_layers", [1, 2])
def test_float64_restatement_of_the_reader_equals_the_fixtures_truth(n_layers):
    g = golden("pillars")
    sd, vox, num, co = _reader_case(g, n_layers)
    assert (num == 1).any() and (num == R.PILLAR["max_points"]).any() and set(co[:, 0].tolist()) == {0, 3}
    truth = g[f"reader{n_layers}_f64"]
    mine = R.reader_f64(sd, vox, num, co, R.PILLAR["voxel_size"], R.PILLAR["pc_range"])
    np.testing.assert_allclose(mine, truth, rtol=1e-11, atol=1e-12)
    y = R.judge(g[f"reader{n_layers}_f32"], truth)
    assert y["dead_ok"] and 1e-8 < y["tensor"] < 1e-6, y        # the yardstick is fp32 rounding, neither 0 nor a bug


@pytest.mark.parametrize("n_layers", [1, 2])
@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_exceed_ten_times_their_bars(n_layers, fault):
    g = golden("pillars")
    sd, vox, num, co = _reader_case(g, n_layers)
    out = R.reader_f64(sd, vox, num, co, R.PILLAR["voxel_size"], R.PILLAR["pc_range"], fault=fault)
    ratio = R.ratios(out, g[f"reader{n_layers}_f32"], g[f"reader{n_layers}_f64"])[0]
    for k in R.MEASURES:
        print(f"{n_layers} layer(s) {fault:20s} {k:9s} ratio {ratio[k]:12.1f}  bar {R.BARS[k]:g}")
        assert ratio[k] > 10 * R.BARS[k], (fault, k, ratio[k])


def test_mean_reader_restatement_equals_the_fixtures_truth():
    g = golden("pillars")
    vp = R.cloud("vn8", 6000, R.VOXELNET, 8)
    n = g["mean_f64"].shape[0]
    vox, num = R.gather(vp, g["vn_c8_rev_index"])[:n], g["vn_c8_rev_num"][:n]
    np.testing.assert_allclose(R.mean_f64(vox, num), g["mean_f64"], rtol=1e-13, atol=0)
    assert R.judge(g["mean_f32"], g["mean_f64"])["tensor"] < 1e-6


def test_fixture_is_arrays_only_and_no_larger_than_the_largest():
    path = os.path.join(ROOT, "tests", "golden", "pillars.npz")
    sizes = [os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
             if f.endswith(".npz") and f != "pillars.npz"]
    assert os.path.getsize(path) <= max(sizes)
    assert all(v.dtype.kind in "fiu" for v in golden("pillars").values())


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dal3.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ENTRIES:
        assert name + "(" in header and name in hip.SIGNATURES and hasattr(lib, name), name
    assert f"#define DAL3_PILLAR_PACK_FLOATS {hip.PILLAR_PACK_FLOATS}" in header
    assert "DAL3_PILLAR_OVERFLOW = 128" in header and hip.PILLAR_OVERFLOW == 128
    assert "dal3_pillars.hip" in open(os.path.join(ROOT, "3dal_pytorch_amd", "csrc", "Makefile")).read()


def test_workspace_sizes_are_the_carve():
    """four (N) key / position arrays, the (256, chunks of 4096) histogram, run starts and ranks (N), the tile counts
    (N / 256), the total and the (B + 1) bases, each padded to 256 bytes"""
    lib = hip.lib()

    def carve(B, N):
        al = lambda b: (b + 255) & ~255
        return 6 * al(4 * N) + al(4 * 256 * ((N + 4095) // 4096)) + al(4 * ((N + 255) // 256)) + al(8) + al(8 * (B + 1))

    assert lib.dal3_voxelize_workspace_bytes(1, 1000) == carve(1, 1000) == 26368
    assert lib.dal3_voxelize_workspace_bytes(4, 720000) == carve(4, 720000) == 17472000
    assert lib.dal3_voxelize_workspace_bytes(-1, 0) == 0 and lib.dal3_voxelize_workspace_bytes(0, 1 << 25) == 0


FAKE = 0x1000                                   # never dereferenced: every case fails before a launch


def _vox_args(off=(0, 40, 100), **kw):
    off = np.asarray(off, np.int64)
    a = hip.VoxelizeArgs(B=off.size - 1, N=100, points=FAKE, point_stride=5, C=5, reverse_index=1, point_offsets=FAKE,
                         point_offsets_host=off.ctypes.data, max_points=20, max_voxels=30, capacity=60, voxels=FAKE,
                         coordinates=FAKE, num_points=FAKE, voxel_offsets=FAKE, status=FAKE, workspace=FAKE, workspace_bytes=1 << 20)
    a.voxel_size[:] = [0.32, 0.32, 4.0]
    a.pc_range[:] = [0.0, -5.12, -3.0, 10.24, 5.12, 1.0]
    a.grid[:] = [32, 32, 1]
    for k, v in kw.items():
        if k in ("voxel_size", "pc_range", "grid"):
            getattr(a, k)[:] = v
        else:
            setattr(a, k, v)
    return a, off


def test_voxelize_argument_errors_without_a_gpu():
    lib = hip.lib()
    assert lib.dal3_voxelize(None, None) == hip.EINVAL and b"null args" in lib.dal3_last_error()
    for kw, what in ((dict(C=2), b"point layout"), (dict(C=9), b"point layout"), (dict(point_stride=4), b"point layout"),
                     (dict(reverse_index=2), b"reverse_index"), (dict(max_points=0), b"max_points"),
                     (dict(max_voxels=0), b"max_voxels"), (dict(grid=[32, 0, 1]), b"grid[1]"),
                     (dict(voxel_size=[0.32, 0.0, 4.0]), b"voxel_size"), (dict(pc_range=[0, float("nan"), 0, 1, 1, 1]), b"pc_range"),
                     (dict(grid=[65536, 65536, 1]), b"2^31"), (dict(voxel_offsets=None), b"null voxel_offsets"),
                     (dict(status=None), b"status"), (dict(point_offsets_host=None), b"point_offsets_host"),
                     (dict(capacity=59), b"capacity 59 too small"), (dict(voxels=None), b"null voxels"),
                     (dict(points=None), b"null points"), (dict(workspace=None), b"workspace")):
        a, off = _vox_args(**kw)
        assert lib.dal3_voxelize(a, None) == hip.EINVAL, kw
        assert what in lib.dal3_last_error(), (kw, lib.dal3_last_error())
    for off in ((0, 50, 40), (0, 40, 101), (-1, 40, 100)):
        a, keepalive = _vox_args(off=off)
        assert lib.dal3_voxelize(a, None) == hip.EINVAL and b"non-decreasing" in lib.dal3_last_error(), off
    a, off = _vox_args(workspace_bytes=16)
    assert lib.dal3_voxelize(a, None) == hip.EWORKSPACE


def test_feature_argument_errors_without_a_gpu():
    lib = hip.lib()
    assert lib.dal3_pillar_features(None, None) == hip.EINVAL

    def args(**kw):
        a = hip.PillarFeatureArgs(P=4, voxels=FAKE, num_points=FAKE, coordinates=FAKE, C=5, max_points=20, n_layers=2, c_out=64,
                                  vx=0.32, vy=0.32, x_offset=0.16, y_offset=-4.96, packed=FAKE, features=FAKE)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw in (dict(C=2), dict(C=9), dict(max_points=0), dict(max_points=65), dict(n_layers=3), dict(c_out=32), dict(packed=None),
               dict(packed=FAKE + 4), dict(features=None), dict(voxels=None), dict(P=-1), dict(canvas=FAKE, ny=0, nx=4, canvas_B=1)):
        assert lib.dal3_pillar_features(args(**kw), None) == hip.EINVAL, kw
    L = hip.Layer(FAKE, None, FAKE, FAKE, FAKE, FAKE, 10, 64)
    assert lib.dal3_pillar_pack(ctypes.byref(L), 1, 6, 1e-3, FAKE, None) == hip.EINVAL and b"11 -> 64" in lib.dal3_last_error()
    assert lib.dal3_pillar_pack(ctypes.byref(L), 3, 5, 1e-3, FAKE, None) == hip.EINVAL
    assert lib.dal3_pillar_pack(ctypes.byref(L), 1, 5, 0.0, FAKE, None) == hip.EINVAL
    assert lib.dal3_pillar_scatter(FAKE, FAKE, 4, None, 64, None, 1, 4, 4, None) == hip.EINVAL
    assert lib.dal3_voxel_mean(None, FAKE, 4, None, 5, 4, FAKE, None) == hip.EINVAL


def test_python_refusals_and_the_modules_keys_without_a_gpu():
    cpu = torch.zeros((8, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pillars.voxelize(cpu, [0, 8], (0.32, 0.32, 4), (0, -5.12, -3, 10.24, 5.12, 1), 20, 100)
    with pytest.raises(TypeError):
        pillars.voxelize(np.zeros((8, 5), np.float32), [0, 8], (0.32, 0.32, 4), (0, -5.12, -3, 10.24, 5.12, 1), 20, 100)
    net = pillars.PillarFeatureNet(num_input_features=5, num_filters=(64, 64), voxel_size=(0.32, 0.32, 6.0),
                                   pc_range=(-74.88, -74.88, -2, 74.88, 74.88, 4.0))
    want = {f"pfn_layers.{i}.{k}" for i in range(2) for k in ("linear.weight", "norm.weight", "norm.bias", "norm.running_mean",
                                                                "norm.running_var", "norm.num_batches_tracked")}
    assert set(net.state_dict()) == want
    net.load_state_dict({k: torch.as_tensor(v) for k, v in R.reader_weights(2, 5).items()}, strict=True)
    assert net.pfn_layers[0].norm.eps == 1e-3 and net.hip_serves(20) and not net.hip_serves(65)
    assert not pillars.PillarFeatureNet(num_input_features=5, with_distance=True).hip_serves(20)
    assert not pillars.PillarFeatureNet(num_input_features=5, num_filters=(32,)).hip_serves(20)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.eval()(torch.zeros(2, 20, 5), torch.ones(2, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32))
    # train mode and the shapes the kernel does not serve are the stock-torch composite: it runs anywhere
    vox, num, co = torch.rand(3, 20, 5), torch.tensor([20, 3, 1]), torch.zeros(3, 4, dtype=torch.int32)
    assert pillars.PillarFeatureNet(num_input_features=5, with_distance=True).eval()(vox, num, co).shape == (3, 64)
    gen = pillars.VoxelGenerator([0.32, 0.32, 6.0], [-74.88, -74.88, -2, 74.88, 74.88, 4.0], 20, max_voxels=[32000, 60000])
    assert gen.grid_size.tolist() == [468, 468, 1] and gen.max_num_points_per_voxel == 20
    assert pillars.capacity_of([0, 5, 5, 4000], 320, [32, 32, 1]) == 5 + 0 + 320


@pytest.mark.parametrize("n_layers", [1, 2])
def test_the_composite_is_the_references_forward(n_layers):
    """what train mode and the unserved shapes run: the reference-keyed weights load strictly and the stock-torch
    composite reproduces the fp32 output the reference's own module recorded"""
    g = golden("pillars")
    sd, vox, num, co = _reader_case(g, n_layers)
    net = pillars.PillarFeatureNet(num_input_features=5, num_filters=(64,) * n_layers, voxel_size=R.PILLAR["voxel_size"],
                                   pc_range=R.PILLAR["pc_range"], norm_cfg=dict(type="BN1d", eps=R.EPS, momentum=0.01)).eval()
    net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    with torch.no_grad():
        out = net.composite(torch.from_numpy(vox), torch.from_numpy(num), torch.from_numpy(co)).numpy()
    want = g[f"reader{n_layers}_f32"]
    assert out.shape == want.shape
    np.testing.assert_allclose(out, want, rtol=1e-5, atol=1e-6)


def test_raw_pointer_arguments_are_checked_before_any_launch():
    """status, point_offsets_device and n_pillars reach the kernels as raw pointers: a host tensor, another dtype or another
    size is refused"""
    f = pillars._device_ints
    dev = torch.device("cpu")
    assert f(None, "n_pillars", torch.int64, 1, dev) is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(torch.zeros(1, dtype=torch.int64), "n_pillars", torch.int64, 1, dev)
    with pytest.raises(TypeError):
        f([3], "n_pillars", torch.int64, 1, dev)
    meta = torch.device("meta")

    class Fake:                                 # a stand-in that says it is on the GPU: only the checks run
        def __init__(self, t):
            self.t, self.is_cuda, self.device, self.dtype = t, True, dev, t.dtype
        numel = lambda self: self.t.numel()
        is_contiguous = lambda self: self.t.is_contiguous()
        shape = property(lambda self: self.t.shape)

    real_is_tensor = torch.is_tensor
    torch.is_tensor = lambda x: isinstance(x, Fake) or real_is_tensor(x)
    try:
        ok = Fake(torch.zeros(1, dtype=torch.int64))
        assert f(ok, "n_pillars", torch.int64, 1, dev) is ok
        for bad in (Fake(torch.zeros(1, dtype=torch.int32)), Fake(torch.zeros(2, dtype=torch.int64)),
                    Fake(torch.zeros((2, 2), dtype=torch.int64)[:, 0])):
            with pytest.raises(ValueError, match="n_pillars must be a contiguous"):
                f(bad, "n_pillars", torch.int64, 1, dev)
        with pytest.raises(ValueError, match="lives on"):
            f(ok, "status", torch.int64, 1, meta)
    finally:
        torch.is_tensor = real_is_tensor


def test_restated_scatter_equals_the_references_canvas():
    g = golden("pillars")
    co = g["batch_coords"][g["reader_rows"]]
    canvas = g["reader2_canvas"]
    assert canvas.shape == (4, 64, 32, 32) and not canvas[1].any() and not canvas[2].any()
    assert np.array_equal(R.scatter(g["reader2_f32"], co, 4, 32, 32).view(np.uint32), canvas.view(np.uint32))


@pytest.mark.parametrize("n_layers", [1, 2])
def test_lane_level_emulation_of_the_feature_kernel_meets_the_bars(n_layers):
    """the kernel's fragment layout, k-step order, butterfly maxima and store pattern restated lane by lane
    (tests/pillars_emu.py), on 16 fixture pillars (one column tile) and on 40-row pillars of 6 features (two tiles)"""
    import pillars_emu as E
    g = golden("pillars")
    sd, vox, num, co = _reader_case(g, n_layers)
    pick = np.arange(0, vox.shape[0], 16)
    P = R.PILLAR
    vx, vy = P["voxel_size"][:2]
    xo, yo = vx / 2 + P["pc_range"][0], vy / 2 + P["pc_range"][1]
    out = E.kernel(E.pack(sd, n_layers, 5, R.EPS), vox[pick], num[pick], co[pick], 5, 20, n_layers, vx, vy, xo, yo)
    ratio = R.ratios(out, g[f"reader{n_layers}_f32"][pick], g[f"reader{n_layers}_f64"][pick])[0]
    print(n_layers, ratio)
    assert all(ratio[k] <= R.BARS[k] for k in R.MEASURES), ratio
    T, C = 40, 6
    u = R.synth.uniform(1, "emu", (6, T, C), -1, 1).astype(np.float32)
    n40 = np.array([1, 40, 39, 33, 32, 7], np.int32)
    u[np.arange(T)[None] >= n40[:, None]] = 0
    c40 = np.array([[0, 0, i, 2 * i] for i in range(6)], np.int32)
    sd6 = R.reader_weights(n_layers, C)
    out = E.kernel(E.pack(sd6, n_layers, C, R.EPS), u, n40, c40, C, T, n_layers, vx, vy, xo, yo)
    j = R.judge(out, R.reader_f64(sd6, u, n40, c40, P["voxel_size"], P["pc_range"]))
    assert j["dead_ok"] and j["tensor"] < 1e-6 and j["chan_max"] < 1e-5, j


def _far_module(n_layers):
    cfg = R.PRODUCTION
    net = pillars.PillarFeatureNet(num_input_features=cfg["C"], num_filters=(64,) * n_layers, voxel_size=cfg["voxel_size"],
                                   pc_range=cfg["pc_range"], norm_cfg=dict(type="BN1d", eps=R.EPS, momentum=0.01)).eval()
    net.load_state_dict({k: torch.as_tensor(v) for k, v in R.reader_weights(n_layers, cfg["C"]).items()}, strict=True)
    return net


@pytest.mark.parametrize("n_layers", [1, 2])
def test_lane_level_emulation_far_from_the_origin_meets_the_bars(n_layers):
    """the production grid's corner, centre and far-corner pillars (x and y indices up to 467, where the decoration
    cancels 74 m against 74 m): the emulation against the float64 truth, the torch-CPU composite as the yardstick, under
    the GPU test's bars, before a GPU is involved"""
    import pillars_emu as E
    cfg = R.PRODUCTION
    vox, num, co = R.far_pillars()
    assert sorted(set(co[:, 3].tolist())) == sorted(set(co[:, 2].tolist())) == list(R.FAR_AT) and (num == 1).any() and (num == 20).any()
    assert np.abs(vox[:, 0, 0]).max() > 74.5 and np.abs(vox[:, 0, 1]).max() > 74.5
    net = _far_module(n_layers)
    sd = R.reader_weights(n_layers, cfg["C"])
    with torch.no_grad():
        f32 = net.composite(torch.from_numpy(vox), torch.from_numpy(num), torch.from_numpy(co)).numpy()
    truth = R.reader_f64(sd, vox, num, co, cfg["voxel_size"], cfg["pc_range"])
    out = E.kernel(E.pack(sd, n_layers, cfg["C"], R.EPS), vox, num, co, cfg["C"], cfg["max_points"], n_layers, net.vx, net.vy,
                   net.x_offset, net.y_offset)
    ratio, m, y = R.ratios(out, f32, truth)
    for k in R.MEASURES:
        print(f"far/l{n_layers} {k:9s} {m[k]:10.3e}  yardstick {y[k]:10.3e}  ratio {ratio[k]:7.2f}  bar {R.BARS[k]:g}")
    assert m["dead_ok"] and all(ratio[k] <= R.BARS[k] for k in R.MEASURES), ratio
