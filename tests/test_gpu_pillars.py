"""The PointPillars reader on the GPU (3dal_pytorch_amd/pillars.py) against what the reference recorded
(tests/golden/pillars.npz) and against tests/pillars_ref.py run on the host.

Voxelisation is exact: voxel count, coordinates, num_points and every row equal the reference's bit for bit. The feature net
is judged per element and per channel against the float64 truth by the rule of tests/test_gpu_f64_parity.py: each measure
<= bar x the torch-CPU fp32 module's own figure on the same rows (pillars_ref.BARS; how they were set is written there).
With DAL3_PILLARS_RECORD=<path> in the environment the run also writes every measure, yardstick and ratio to <path>
(tests/pillars_gpu.py; how profiles/pillars_measured.json was made)."""
import copy
import importlib

import numpy as np
import pytest
import torch

import pillars_ref as R
from _common import golden
from pillars_gpu import _dev, _hold, _module, _record_file, _run, _same       # _record_file: the autouse fixture

hip = importlib.import_module("3dal_pytorch_amd._hip")
pillars = importlib.import_module("3dal_pytorch_amd.pillars")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return golden("pillars")


def _single(g, name):
    if name in R.PILLAR_CAPS:
        return R.cloud(f"pillar{int(g['pillar_salt'])}", 20000, R.PILLAR, R.PILLAR["C"]), R.PILLAR, R.PILLAR_CAPS[name], True
    C, rev = R.VOXELNET_CASES[name]
    return R.cloud(f"vn{C}", 6000, R.VOXELNET, C), R.VOXELNET, R.VOXELNET["max_voxels"], rev


@pytest.mark.parametrize("name", sorted(R.PILLAR_CAPS) + sorted(R.VOXELNET_CASES))
def test_voxelisation_equals_the_reference_exactly(g, name):
    pts, cfg, cap, rev = _single(g, name)
    (voxels, coords, num, nv), _ = _run(pts, [0, pts.shape[0]], cfg, cap, rev)
    want_num = g[name + "_num"]
    assert nv.tolist() == [want_num.size] and not coords[:, 0].any()
    _same((voxels, coords[:, 1:], num), (R.gather(pts, g[name + "_index"]), g[name + "_coords"], want_num))


def test_voxelisation_of_the_ragged_batch_equals_the_reference_exactly(g):
    pts, off = R.batch_points()
    (voxels, coords, num, nv), r = _run(pts, off, R.PILLAR, R.BATCH_CAP)
    assert nv.tolist() == g["batch_num_voxels"].tolist() and nv[1] == 0 and nv[2] == 0
    assert r.voxel_offsets.cpu().tolist() == np.concatenate([[0], np.cumsum(nv)]).tolist()
    _same((voxels, coords, num), (R.gather(pts, g["batch_index"]), g["batch_coords"], g["batch_num"]))


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 9001])
def test_point_counts_around_the_tile_and_over_several_chunks(n):
    """9001 points: three sort chunks of 4096; max_workgroups=2 makes every workgroup walk more than one tile / chunk"""
    pts = R.cloud(f"count{n}", n, R.PILLAR, 5) if n else np.zeros((0, 5), np.float32)
    want = R.voxelize_batch(pts, [0, n], R.PILLAR["voxel_size"], R.PILLAR["pc_range"], R.PILLAR["max_points"], 200)
    for mw in (0, 2):
        got, _ = _run(pts, [0, n], R.PILLAR, 200, max_workgroups=mw)
        _same(got, want)
    assert n < 9001 or want[3][0] == 200


def test_a_sample_is_independent_of_its_batch_and_of_the_run():
    cfg = R.PILLAR
    a = R.cloud("indep/a", 5000, cfg, 5)
    others = [R.cloud("indep/b", 3000, cfg, 5), R.cloud("indep/c", 1234, cfg, 5)]
    alone, _ = _run(a, [0, 5000], cfg, 300)
    again, _ = _run(a, [0, 5000], cfg, 300)
    _same(again, alone)
    for order in ([a] + others, others + [a]):
        off = np.concatenate([[0], np.cumsum([p.shape[0] for p in order])])
        (voxels, coords, num, nv), _ = _run(np.concatenate(order), off, cfg, 300)
        b = 0 if order[0] is a else 2
        rows = coords[:, 0] == b
        assert nv[b] == alone[3][0]
        _same((voxels[rows], coords[rows, 1:], num[rows]), (alone[0], alone[1][:, 1:], alone[2]))
    # a strided point table is read in place
    wide = np.zeros((5000, 8), np.float32)
    wide[:, :5] = a
    r = pillars.voxelize(_dev(wide)[:, :5], [0, 5000], cfg["voxel_size"], cfg["pc_range"], cfg["max_points"], 300)
    _same([t.cpu().numpy() for t in r.finish()[:3]], alone[:3])


def _reader_inputs(g):
    pts, off = R.batch_points()
    rows = g["reader_rows"]
    return R.gather(pts, g["batch_index"])[rows], g["batch_num"][rows], g["batch_coords"][rows]


@pytest.mark.parametrize("n_layers", [1, 2])
def test_reader_against_the_float64_truth_per_element_and_per_channel(g, n_layers):
    vox, num, co = _reader_inputs(g)
    out = _module(n_layers)(_dev(vox), _dev(num), _dev(co))
    assert out.shape == (vox.shape[0], 64)
    _hold(f"reader{n_layers}", out.cpu().numpy(), g[f"reader{n_layers}_f32"], g[f"reader{n_layers}_f64"])


@pytest.mark.parametrize("max_points,C", [(1, 3), (31, 4), (32, 8), (33, 5), (64, 6)])
def test_reader_at_other_row_counts_and_widths(max_points, C):
    """one and two column tiles, a tile that is exactly full, every k-step count of the first layer; judged against the
    float64 restatement with the torch-CPU fp32 module (the composite, which IS the reference's forward) as the yardstick"""
    P = 37
    u = R.synth.uniform(R.SEED, f"rows{max_points}/{C}", (P, max_points, C), -1.0, 1.0).astype(np.float32)
    num = (1 + (np.arange(P) * 7) % max_points).astype(np.int32)
    num[:3] = [1, max_points, max(1, max_points - 1)]
    u[np.arange(max_points)[None, :] >= num[:, None]] = 0
    co = np.stack([np.zeros(P), np.zeros(P), np.arange(P) % 32, (np.arange(P) * 5) % 32], 1).astype(np.int32)
    u[:, :, 0] += (co[:, 3:4] * 0.32).astype(np.float32)
    u[np.arange(max_points)[None, :] >= num[:, None]] = 0
    for n_layers in (1, 2):
        net = _module(n_layers, C)
        out = net(_dev(u), _dev(num), _dev(co)).cpu().numpy()
        sd = R.reader_weights(n_layers, C)
        truth = R.reader_f64(sd, u, num, co, R.PILLAR["voxel_size"], R.PILLAR["pc_range"])
        with torch.no_grad():
            f32 = net.cpu().composite(torch.from_numpy(u), torch.from_numpy(num), torch.from_numpy(co)).numpy()
        _hold(f"rows{max_points}/c{C}/l{n_layers}", out, f32, truth)


@pytest.mark.parametrize("P", [0, 1, 3, 4, 5, 4 * 4096 - 1, 4 * 4096 + 1])
def test_pillar_counts_around_the_tile_and_a_workgroups_share(g, P):
    """a workgroup takes four pillars at a time and the grid is capped at 4096 workgroups: either side of both, and the
    same pillar gives the same bits wherever it sits"""
    vox, num, co = _reader_inputs(g)
    net = _module(2)
    base = net(_dev(vox), _dev(num), _dev(co)).cpu().numpy()
    pick = np.arange(P) % vox.shape[0]
    out = net(_dev(vox[pick]), _dev(num[pick]), _dev(co[pick]))
    assert out.shape == (P, 64)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), base[pick].view(np.uint32))


def test_canvas_routes_give_the_same_bits(g):
    pts, off = R.batch_points()
    cfg = R.PILLAR
    grid = R.grid_of(cfg["voxel_size"], cfg["pc_range"])
    nx, ny, B = int(grid[0]), int(grid[1]), len(off) - 1
    net = _module(2)
    r = pillars.voxelize(_dev(pts), off, cfg["voxel_size"], cfg["pc_range"], cfg["max_points"], R.BATCH_CAP)
    voxels, coords, num, nv = r.finish()
    feats = net(voxels, num, coords)
    two_step = pillars.PointPillarsScatter(64)(feats, coords, B, [nx, ny])
    fused = net.forward_canvas(voxels, num, coords, B, [nx, ny])
    capacity_sized = net.forward_canvas(r.voxels, r.num_points, r.coordinates, B, [nx, ny], n_pillars=r.n_pillars)
    reader = pillars.PillarReader(dict(voxel_size=cfg["voxel_size"], pc_range=cfg["pc_range"], max_points=cfg["max_points"],
                                       max_voxels=R.BATCH_CAP, num_input_features=5, norm_cfg=dict(type="BN1d", eps=R.EPS, momentum=0.01)))
    reader.reader.load_state_dict(net.state_dict(), strict=True)
    whole = reader.cuda().eval()(_dev(pts), off)
    resident = reader(_dev(pts), off, point_offsets_device=_dev(off))
    with pytest.raises(ValueError, match="n_pillars must be a contiguous"):
        net.forward_canvas(r.voxels, r.num_points, r.coordinates, B, [nx, ny], n_pillars=r.n_pillars.to(torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pillars.voxelize(_dev(pts), off, cfg["voxel_size"], cfg["pc_range"], cfg["max_points"], R.BATCH_CAP, status=torch.zeros(1, dtype=torch.int32))
    want = R.scatter(feats.cpu().numpy(), coords.cpu().numpy(), B, ny, nx)
    assert two_step.shape == (B, 64, ny, nx) and int(nv.sum()) < B * ny * nx
    for canvas in (two_step, fused, capacity_sized, whole, resident):
        assert np.array_equal(canvas.cpu().numpy().view(np.uint32), want.view(np.uint32))      # +0 bit for bit where no pillar is
    # the reference's own canvas of the fixture rows: +0 wherever it has no pillar, its cells judged like the rows
    vox, num, co = _reader_inputs(g)
    mine = net.forward_canvas(_dev(vox), _dev(num), _dev(co), B, [nx, ny]).cpu().numpy()
    ref_canvas = g["reader2_canvas"]
    empty = np.ones((B, ny, nx), bool)
    empty[co[:, 0], co[:, 2], co[:, 3]] = False
    assert not mine.transpose(0, 2, 3, 1)[empty].view(np.uint32).any() and not ref_canvas.transpose(0, 2, 3, 1)[empty].any()
    cells = lambda c: c[co[:, 0], :, co[:, 2], co[:, 3]]
    assert np.array_equal(cells(ref_canvas), g["reader2_f32"])
    _hold("reader2/canvas", cells(mine), cells(ref_canvas), g["reader2_f64"])
    # and the rows the fixture holds are the rows judged above
    rows = torch.as_tensor(g["reader_rows"].astype(np.int64)).cuda()
    _hold("reader2/from_voxelize", feats[rows].cpu().numpy(), g["reader2_f32"], g["reader2_f64"])


def test_mean_reader(g):
    vp = R.cloud("vn8", 6000, R.VOXELNET, 8)
    n = g["mean_f64"].shape[0]
    vox, num = R.gather(vp, g["vn_c8_rev_index"])[:n], g["vn_c8_rev_num"][:n]
    out = pillars.VoxelFeatureExtractorV3(num_input_features=8)(_dev(vox), _dev(num)).cpu().numpy()
    _hold("mean", out, g["mean_f32"], g["mean_f64"])


def _plain_train_forward(sd, vox, num, co):
    """PillarFeatureNet in TRAIN mode as a plain torch formulation on the CPU, written from the definition (Linear, then
    nn.BatchNorm1d over (P, C, T) in train mode, ReLU, max over the rows, the repeated maximum appended) -> (output, the
    BatchNorms after the step)"""
    x = torch.from_numpy(vox)
    P, T, _ = x.shape
    vx, vy = R.PILLAR["voxel_size"][:2]
    xo, yo = vx / 2 + R.PILLAR["pc_range"][0], vy / 2 + R.PILLAR["pc_range"][1]
    n = torch.from_numpy(num)
    c = torch.from_numpy(co).float()
    mean = x[:, :, :3].sum(1, keepdim=True) / n.float().view(-1, 1, 1)
    rows = torch.cat([x, x[:, :, :3] - mean, (x[:, :, 0] - (c[:, 3:4] * vx + xo)).unsqueeze(2),
                      (x[:, :, 1] - (c[:, 2:3] * vy + yo)).unsqueeze(2)], 2)
    rows = rows * (torch.arange(T).view(1, T) < n.view(-1, 1)).float().unsqueeze(2)
    n_layers = sum(1 for k in sd if k.endswith("linear.weight"))
    bns = []
    with torch.no_grad():
        for i in range(n_layers):
            p = f"pfn_layers.{i}."
            w = torch.from_numpy(sd[p + "linear.weight"])
            bn = torch.nn.BatchNorm1d(w.shape[0], eps=R.EPS, momentum=0.01)
            bn.load_state_dict({k: torch.as_tensor(sd[p + "norm." + k]) for k in ("weight", "bias", "running_mean", "running_var",
                                                                                   "num_batches_tracked")})
            bn.train()
            y = torch.relu(bn((rows @ w.t()).permute(0, 2, 1))).permute(0, 2, 1)
            top = y.max(1, keepdim=True)[0]
            rows = top if i == n_layers - 1 else torch.cat([y, top.repeat(1, T, 1)], 2)
            bns.append(bn)
    return rows.reshape(P, -1).numpy(), bns


def test_drop_in_state_dict_and_the_composite_routes(g):
    vox, num, co = _reader_inputs(g)
    net = _module(2)
    hip_out = net(_dev(vox), _dev(num), _dev(co))
    # the composite (what train mode and with_distance run) is the reference's forward: it matches the fixture's fp32 module
    with torch.no_grad():
        comp = net.composite(_dev(vox), _dev(num), _dev(co))
    np.testing.assert_allclose(comp.cpu().numpy(), g["reader2_f32"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(hip_out.cpu().numpy(), comp.cpu().numpy(), rtol=1e-4, atol=1e-5)
    # train mode takes the composite: batch statistics in the forward, running statistics moved, as a plain torch module
    # on the CPU in train mode does (a copy of the net: train mode moves the statistics)
    tr = copy.deepcopy(net).train()
    out = tr(_dev(vox), _dev(num), _dev(co))
    assert out.requires_grad and out.shape == (vox.shape[0], 64)
    want, bns = _plain_train_forward(R.reader_weights(2, 5), vox, num, co)
    np.testing.assert_allclose(out.detach().cpu().numpy(), want, rtol=1e-4, atol=1e-5)
    assert not np.allclose(want, g["reader2_f32"], rtol=1e-2, atol=1e-3)           # batch statistics, not the running ones
    for layer, bn in zip(tr.pfn_layers, bns):
        np.testing.assert_allclose(layer.norm.running_mean.cpu().numpy(), bn.running_mean.numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(layer.norm.running_var.cpu().numpy(), bn.running_var.numpy(), rtol=1e-5, atol=1e-6)
        assert int(layer.norm.num_batches_tracked) == int(bn.num_batches_tracked) == 8
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in tr.parameters())
    assert np.array_equal(net(_dev(vox), _dev(num), _dev(co)).cpu().numpy(), hip_out.cpu().numpy())
    # a changed weight is repacked
    with torch.no_grad():
        net.pfn_layers[1].norm.bias.add_(1.0)
    assert not np.array_equal(net(_dev(vox), _dev(num), _dev(co)).cpu().numpy(), hip_out.cpu().numpy())
    dist = pillars.PillarFeatureNet(num_input_features=5, num_filters=(64,), with_distance=True, voxel_size=R.PILLAR["voxel_size"],
                                    pc_range=R.PILLAR["pc_range"]).cuda().eval()
    with torch.no_grad():
        a = dist(_dev(vox), _dev(num), _dev(co))
        b = dist.cpu()(torch.from_numpy(vox), torch.from_numpy(num), torch.from_numpy(co))
    np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=1e-4, atol=1e-5)
    # VoxelGenerator: one sample, the reference's three arrays
    pts = R.cloud(f"pillar{int(g['pillar_salt'])}", 20000, R.PILLAR, 5)
    gen = pillars.VoxelGenerator(R.PILLAR["voxel_size"], R.PILLAR["pc_range"], R.PILLAR["max_points"], max_voxels=600)
    voxels, coords, num3 = gen.generate(_dev(pts))
    _same((voxels.cpu().numpy(), coords.cpu().numpy(), num3.cpu().numpy()),
          (R.gather(pts, g["cap600_index"]), g["cap600_coords"], g["cap600_num"]))
