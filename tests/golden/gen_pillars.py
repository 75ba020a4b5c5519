#!/usr/bin/env python3
"""Generate tests/golden/pillars.npz from the REAL reference (jacky121298/3DAL_PyTorch): its own `points_to_voxel`
(det3d/ops/point_cloud/point_cloud_ops.py) through `VoxelGenerator.generate` (det3d/core/input/voxel_generator.py),
`PillarFeatureNet` and `PointPillarsScatter` (det3d/models/readers/pillar_encoder.py) and `VoxelFeatureExtractorV3`
(det3d/models/readers/voxel_encoder.py), on the seeded inputs of tests/pillars_ref.py (rebuilt from their seeds where the
fixture is used).

Run only where the reference checkout exists (DAL3_REFERENCE, default /root/reference):
    python tests/golden/gen_pillars.py

The four files are loaded by path behind stub modules for what their import chain needs and this machine lacks: numba
with `jit` as identity (the voxeliser then runs as plain Python), the registries, and det3d.models.utils with
`get_paddings_indicator` and `build_norm_layer` restated (BN1d -> nn.BatchNorm1d with the cfg's eps and momentum).

What is recorded. A voxelisation is stored as WHICH point sits at each row (an index map, recovered from the reference's
own voxels by looking each row up among the input points, whose rows are unique; -1 = padding), its coordinates and
num_points: the voxels are the input points gathered through it, and that gather is asserted here to equal the reference's
voxels bit for bit. The NaN points of a cloud are left out of the reference's input (it casts them to an index); the
indices stored are those of the full cloud. The reader is recorded on a subset of the batch's pillars (`reader_rows`): the
fp32 modules' outputs, the same modules' .double() outputs as the truth; the reference's PointPillarsScatter canvas of the two-layer features is stored (`reader2_canvas`, mostly zeros) and
asserted here to equal pillars_ref.scatter of them. The archive is written with fixed timestamps, so a rerun
reproduces it byte for byte.
"""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import pillars_ref as R  # noqa: E402

REF = os.environ.get("DAL3_REFERENCE", "/root/reference")
READER_ROWS = 256


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    mod.__path__ = []
    mod.__dict__.update(attrs)
    sys.modules[name] = mod
    return mod


def _load_file(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_reference():
    def jit(*args, **kwargs):
        return args[0] if args and callable(args[0]) else (lambda fn: fn)

    class Registry:
        @staticmethod
        def register_module(cls):
            return cls

    def get_paddings_indicator(actual_num, max_num, axis=0):
        actual_num = torch.unsqueeze(actual_num, axis + 1)
        shape = [1] * len(actual_num.shape)
        shape[axis + 1] = -1
        max_num = torch.arange(max_num, dtype=torch.int, device=actual_num.device).view(shape)
        return actual_num.int() > max_num

    def build_norm_layer(cfg, num_features, postfix=""):
        assert cfg["type"] == "BN1d"
        return "bn" + str(postfix), nn.BatchNorm1d(num_features, eps=cfg.get("eps", 1e-5), momentum=cfg.get("momentum", 0.1))

    _stub("numba", jit=jit)
    for name in ["det3d", "det3d.ops", "det3d.ops.point_cloud", "det3d.core", "det3d.core.input", "det3d.models",
                 "det3d.models.readers"]:
        _stub(name)
    _stub("det3d.models.registry", BACKBONES=Registry, READERS=Registry)
    _stub("det3d.models.utils", get_paddings_indicator=get_paddings_indicator, build_norm_layer=build_norm_layer)
    _load_file("det3d.ops.point_cloud.point_cloud_ops", "det3d/ops/point_cloud/point_cloud_ops.py")
    gen = _load_file("det3d.core.input.voxel_generator", "det3d/core/input/voxel_generator.py")
    pil = _load_file("det3d.models.readers.pillar_encoder", "det3d/models/readers/pillar_encoder.py")
    vox = _load_file("det3d.models.readers.voxel_encoder", "det3d/models/readers/voxel_encoder.py")
    return gen, pil, vox


def index_of(points, voxels, num):
    """which point each row of the reference's voxels is: looked up by the row's bytes"""
    finite = ~np.isnan(points[:, :3]).any(1)
    table = {}
    for i in np.nonzero(finite)[0]:
        key = points[i].tobytes()
        assert key not in table, "two input points are identical: the fixture could not tell them apart"
        table[key] = int(i)
    index = -np.ones(voxels.shape[:2], np.int32)
    for v in range(voxels.shape[0]):
        for r in range(int(num[v])):
            index[v, r] = table[voxels[v, r].tobytes()]
        assert not voxels[v, int(num[v]):].any()
    return index


def reference_voxels(gen, points, cfg, max_voxels, reverse=True):
    """the reference on the cloud without its NaN points -> (index into the FULL cloud, coords (M, 3), num)"""
    g = gen.VoxelGenerator(cfg["voxel_size"], cfg["pc_range"], cfg["max_points"], max_voxels)
    clean = R.drop_nan(points)
    if reverse:
        voxels, coords, num = g.generate(clean)
    else:
        from det3d.ops.point_cloud.point_cloud_ops import points_to_voxel
        voxels, coords, num = points_to_voxel(clean, g.voxel_size, g.point_cloud_range, cfg["max_points"], False, max_voxels)
    index = index_of(points, voxels, num)
    assert np.array_equal(R.gather(points, index).view(np.uint32), voxels.view(np.uint32))
    return index, coords.astype(np.int32), num.astype(np.int32)


def checksum(points):
    return float(np.nan_to_num(points.astype(np.float64), nan=3.0, posinf=5.0, neginf=7.0).sum())


def module_outputs(mod, voxels, num, coords):
    with torch.no_grad():
        co = None if coords is None else torch.from_numpy(coords)
        f32 = mod(torch.from_numpy(voxels), torch.from_numpy(num), co)
        f64 = mod.double()(torch.from_numpy(voxels).double(), torch.from_numpy(num), co)
        mod.float()
    return f32.reshape(voxels.shape[0], -1).numpy(), f64.reshape(voxels.shape[0], -1).numpy()


def save(path, arrays):
    """np.load-compatible, with fixed timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            a = np.asarray(arrays[name])
            np.lib.format.write_array(buf, a if a.ndim == 0 else np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    gen, pil, vox = import_reference()
    out = {}
    # ---- the pillar grid, one cloud, three caps
    P = R.PILLAR
    for salt in range(200):                     # a cloud with pillars of 1, exactly max_points and more points
        pts = R.cloud(f"pillar{salt}", 20000, P, P["C"])
        ok, c = R.cells(pts, P["voxel_size"], P["pc_range"])
        per_cell = np.unique(c[ok] @ np.array([1, 1000, 1000000]), return_counts=True)[1]
        if (per_cell == 1).any() and (per_cell == P["max_points"]).any() and (per_cell > P["max_points"]).any():
            break
    else:
        raise RuntimeError("no cloud with pillars of 1, exactly max_points and more than max_points points")
    out["pillar_salt"] = np.asarray(salt, np.int64)
    out["pillar_sum"] = np.asarray(checksum(pts))
    for name, cap in R.PILLAR_CAPS.items():
        index, coords, num = reference_voxels(gen, pts, P, cap)
        print(f"pillar {name}: cap {cap}, {num.size} voxels of {per_cell.size} occupied cells, {int((num == 20).sum())} full")
        assert (num.size < cap) if name == "free" else (num.size == cap and per_cell.size > cap)
        mine = R.voxelize_index(pts, P["voxel_size"], P["pc_range"], P["max_points"], cap)
        assert np.array_equal(mine[0], index) and np.array_equal(mine[1][:, ::-1], coords) and np.array_equal(mine[2], num)
        out.update({f"{name}_index": index, f"{name}_coords": coords, f"{name}_num": num})
    # ---- the ragged batch
    bpts, off = R.batch_points()
    out["batch_sum"] = np.asarray(checksum(bpts))
    bi, bc, bn, bnv = [], [], [], []
    for b in range(len(off) - 1):
        sample = bpts[off[b]:off[b + 1]]
        index, coords, num = reference_voxels(gen, sample, P, R.BATCH_CAP)
        bi.append(np.where(index >= 0, index + off[b], -1).astype(np.int32))
        bc.append(np.concatenate([np.full((coords.shape[0], 1), b, np.int32), coords], 1))     # collate_kitti's pad
        bn.append(num)
        bnv.append(num.size)
    assert bnv[1] == 0 and bnv[2] == 0 and bnv[0] == R.BATCH_CAP and 0 < bnv[3] < R.BATCH_CAP, bnv
    out.update(batch_index=np.concatenate(bi), batch_coords=np.concatenate(bc), batch_num=np.concatenate(bn),
               batch_num_voxels=np.asarray(bnv, np.int64))
    print(f"batch: counts {R.BATCH_COUNTS}, voxels {bnv}")
    # ---- the VoxelNet-style grid
    V = R.VOXELNET
    for name, (C, reverse) in R.VOXELNET_CASES.items():
        vp = R.cloud(f"vn{C}", 6000, V, C)
        out[f"{name}_sum"] = np.asarray(checksum(vp))
        index, coords, num = reference_voxels(gen, vp, V, V["max_voxels"], reverse)
        assert num.size == V["max_voxels"] and (num == V["max_points"]).any() and (num < V["max_points"]).any()
        out.update({f"{name}_index": index, f"{name}_coords": coords, f"{name}_num": num})
        print(f"voxelnet {name}: {num.size} voxels, z cells {sorted(set(coords[:, 0 if reverse else 2].tolist()))}")
    # ---- the reader, on a subset of the batch's pillars
    voxels = R.gather(bpts, out["batch_index"])
    coords, num = out["batch_coords"], out["batch_num"]
    M = num.size
    rows = np.unique(np.concatenate([np.linspace(0, M - 1, READER_ROWS).astype(np.int64), np.nonzero(num == 1)[0][:8],
                                     np.nonzero(num == P["max_points"])[0][:8]]))[:READER_ROWS]
    assert (num[rows] == 1).any() and (num[rows] == P["max_points"]).any() and len(set(coords[rows, 0].tolist())) == 2
    out["reader_rows"] = rows.astype(np.int32)
    grid = R.grid_of(P["voxel_size"], P["pc_range"])
    for n_layers in (1, 2):
        sd = R.reader_weights(n_layers, P["C"])
        mod = pil.PillarFeatureNet(num_input_features=P["C"], num_filters=(64,) * n_layers, voxel_size=P["voxel_size"],
                                   pc_range=P["pc_range"], norm_cfg=dict(type="BN1d", eps=R.EPS, momentum=0.01)).eval()
        mod.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
        f32, f64 = module_outputs(mod, voxels[rows], num[rows], coords[rows])
        mine = R.reader_f64(sd, voxels[rows], num[rows], coords[rows], P["voxel_size"], P["pc_range"])
        assert np.allclose(mine, f64, rtol=1e-11, atol=1e-12), np.abs(mine - f64).max()
        y = R.judge(f32, f64)
        print(f"reader {n_layers} layer(s): {rows.size} pillars, |out| max {np.abs(f64).max():.3f}, fp32 own error {y}")
        out[f"reader{n_layers}_f32"], out[f"reader{n_layers}_f64"] = f32.astype(np.float32), f64
        canvas = pil.PointPillarsScatter(num_input_features=64)(torch.from_numpy(f32), torch.from_numpy(coords[rows]), 4,
                                                                [int(grid[0]), int(grid[1])]).numpy()
        assert np.array_equal(canvas.view(np.uint32), R.scatter(f32, coords[rows], 4, int(grid[1]), int(grid[0])).view(np.uint32))
        if n_layers == 2:
            out["reader2_canvas"] = canvas
    # ---- the mean reader, on a VoxelNet case
    vp = R.cloud("vn8", 6000, V, 8)
    vv = R.gather(vp, out["vn_c8_rev_index"])[:READER_ROWS]
    vn = out["vn_c8_rev_num"][:READER_ROWS]
    m32, m64 = module_outputs(vox.VoxelFeatureExtractorV3(num_input_features=8), vv, vn, None)
    assert np.allclose(R.mean_f64(vv, vn), m64, rtol=1e-13, atol=0)
    out["mean_f32"], out["mean_f64"] = m32.astype(np.float32), m64
    path = os.path.join(HERE, "pillars.npz")
    save(path, out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
