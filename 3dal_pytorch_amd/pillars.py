"""The PointPillars reader on the GPU through lib3dal_hip.so (dal3_voxelize, dal3_pillar_features, dal3_pillar_scatter,
dal3_voxel_mean, include/dal3.h), under the reference's names: `points_to_voxel`'s result through `voxelize` /
`VoxelGenerator` (det3d/ops/point_cloud/point_cloud_ops.py:7-184, det3d/core/input/voxel_generator.py), `PillarFeatureNet`
and `PointPillarsScatter` (det3d/models/readers/pillar_encoder.py:15-209), `VoxelFeatureExtractorV3`
(det3d/models/readers/voxel_encoder.py:9-24), and `PillarReader`: points + offsets -> the BEV canvas in one enqueue with no
host synchronisation.

The voxelisation is defined exactly in include/dal3.h and equals the reference's sequential loop bit for bit (tests/
pillars_ref.py restates it); its one departure: a point with a NaN coordinate is dropped (the reference casts the NaN to an
index). Sizes are never known only after the run: the outputs are capacity-sized, the samples' voxels packed back to back
with a device `voxel_offsets`, and `VoxelizeResult.finish()` — the one host synchronisation — trims them to the collated
batch's shapes. `PillarFeatureNet.forward` always returns (P, C_out): the reference's `features.squeeze()` turns P = 1 into
a vector, this does not.
"""
import numpy as np
import torch
from torch import nn

from . import _hip


def grid_size(voxel_size, pc_range):
    """round((hi - lo) / size) in float32, as VoxelGenerator and points_to_voxel form it -> (3,) int64 [x, y, z]"""
    r = np.asarray(pc_range, dtype=np.float32)
    v = np.asarray(voxel_size, dtype=np.float32)
    return np.round((r[3:] - r[:3]) / v).astype(np.int64)


def capacity_of(point_offsets, max_voxels, grid):
    """rows the packed outputs need: the samples' min(points, max_voxels, cells) summed"""
    n = np.diff(np.asarray(point_offsets, dtype=np.int64).reshape(-1))
    return int(np.minimum(n, min(int(max_voxels), int(np.prod(np.asarray(grid, dtype=np.int64))))).sum())


def _alloc(allocator, nbytes, device):
    if allocator is not None:
        ws = allocator(nbytes)
        _hip.require_gpu(ws, "workspace")
        if ws.dtype != torch.uint8 or ws.numel() < nbytes or not ws.is_contiguous():
            raise ValueError(f"the allocator must return a contiguous uint8 tensor of at least {nbytes} bytes")
        return ws
    return _hip.workspace(nbytes, device)


def _device_ints(t, what, dtype, count, device):
    """a caller's tensor that a kernel reads or writes through its raw pointer: on `device`, contiguous, `dtype`, `count`
    elements; None passes"""
    if t is None:
        return None
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor")
    _hip.require_gpu(t, what)
    if t.device != device:
        raise ValueError(f"{what} lives on {t.device}, the other inputs on {device}")
    if t.dtype != dtype or t.numel() != count or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {dtype} tensor of {count} element(s), got {t.dtype} {tuple(t.shape)}")
    return t


class VoxelizeResult:
    """The device tensors of one `voxelize` call: voxels (capacity, max_points, C), coordinates (capacity, 4) int32 [b, z, y, x]
    (or [b, x, y, z]), num_points (capacity) int32, voxel_offsets (B + 1) int64, status (1) int32. Rows from
    voxel_offsets[B] on are zero. `n_pillars` is the one-element view voxel_offsets[B:] the later kernels read."""

    def __init__(self, voxels, coordinates, num_points, voxel_offsets, status, B):
        self.voxels, self.coordinates, self.num_points = voxels, coordinates, num_points
        self.voxel_offsets, self.status, self.B = voxel_offsets, status, B

    @property
    def n_pillars(self):
        return self.voxel_offsets[self.B:]

    def finish(self):
        """-> voxels (M, max_points, C), coordinates (M, 4), num_points (M), num_voxels (B) int64: the collated batch. The one
        host synchronisation."""
        off = self.voxel_offsets.cpu()
        if int(self.status.item()) & _hip.PILLAR_OVERFLOW:
            raise RuntimeError("voxelize: the device point_offsets disagree with the host's (status DAL3_PILLAR_OVERFLOW)")
        m = int(off[-1])
        return self.voxels[:m], self.coordinates[:m], self.num_points[:m], (off[1:] - off[:-1]).to(self.voxels.device)


def voxelize(points, point_offsets, voxel_size, pc_range, max_points, max_voxels, reverse_index=True, *, status=None,
             point_offsets_device=None, allocator=None, max_workgroups=0):
    """points (N, C) float32 CUDA, 3 <= C <= 8, rows with stride(1) == 1; point_offsets (B + 1) on the HOST: sample b is rows
    [point_offsets[b], point_offsets[b + 1]). -> VoxelizeResult, enqueued on the current stream, no synchronisation.
    point_offsets_device: the same offsets as a CUDA int64 (B + 1) tensor; without it they are uploaded here, a small copy
    from pageable host memory. status: a CUDA int32 (1) tensor the kernels OR problems into (_hip.PILLAR_OVERFLOW).
    allocator: bytes -> a uint8 CUDA tensor for the workspace (torch.empty otherwise)."""
    if not torch.is_tensor(points):
        raise TypeError("points must be a tensor")
    _hip.require_gpu(points, "points")
    if points.dim() != 2 or not 3 <= points.shape[1] <= 8:
        raise ValueError(f"points must be (N, 3 .. 8), got {tuple(points.shape)}")
    if points.dtype != torch.float32:
        raise TypeError(f"points must be float32, got {points.dtype}")
    N, C = points.shape
    if N and (points.stride(1) != 1 or points.stride(0) < C):
        points = points.contiguous()
    off = _hip.host_offsets(point_offsets, N, "point_offsets", "the capacity of the outputs comes", "B")
    B = off.size - 1
    max_points, max_voxels = int(max_points), int(max_voxels)
    if max_points < 1 or max_voxels < 1:
        raise ValueError("max_points and max_voxels must be >= 1")
    vs = np.asarray(voxel_size, dtype=np.float32).reshape(-1)
    rng = np.asarray(pc_range, dtype=np.float32).reshape(-1)
    if vs.size != 3 or rng.size != 6:
        raise ValueError("voxel_size needs 3 entries and pc_range 6")
    grid = grid_size(vs, rng)
    if np.any(grid < 1):
        raise ValueError(f"the grid {grid.tolist()} has an axis without a cell")
    if B * int(np.prod(grid)) >= 2 ** 31 - 1:
        raise ValueError(f"B * cells = {B} * {int(np.prod(grid))} does not fit the 31-bit (sample, cell) key: split the batch")
    dev = points.device
    cap = capacity_of(off, max_voxels, grid)
    voxels = torch.empty((cap, max_points, C), dtype=torch.float32, device=dev)
    coords = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    num = torch.empty(cap, dtype=torch.int32, device=dev)
    vo = torch.empty(B + 1, dtype=torch.int64, device=dev)
    status = _device_ints(status, "status", torch.int32, 1, dev)
    off_dev = _device_ints(point_offsets_device, "point_offsets_device", torch.int64, B + 1, dev)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    if off_dev is None:
        off_dev = torch.from_numpy(off).to(dev)         # a small upload from pageable memory: pass point_offsets_device to avoid it
    lib = _hip.lib()
    nbytes = lib.dal3_voxelize_workspace_bytes(B, N)
    ws = _alloc(allocator, nbytes, dev)
    a = _hip.VoxelizeArgs(B=B, N=N, points=_hip.ptr(points), point_stride=points.stride(0) if N else C, C=C,
                          reverse_index=1 if reverse_index else 0, point_offsets=_hip.ptr(off_dev),
                          point_offsets_host=off.ctypes.data, max_points=max_points, max_voxels=max_voxels, capacity=cap,
                          voxels=_hip.ptr(voxels), coordinates=_hip.ptr(coords), num_points=_hip.ptr(num),
                          voxel_offsets=_hip.ptr(vo), status=_hip.ptr(status), max_workgroups=int(max_workgroups),
                          workspace=_hip.ptr(ws), workspace_bytes=nbytes)
    a.voxel_size[:] = vs.tolist()
    a.pc_range[:] = rng.tolist()
    a.grid[:] = [int(g) for g in grid]
    _hip.check(lib.dal3_voxelize(a, _hip.stream()))
    return VoxelizeResult(voxels, coords, num, vo, status, B)


def double_flip(points, point_offsets, point_offsets_device=None, *, max_workgroups=0):
    """DoubleFlip (det3d/datasets/pipelines/test_aug.py) on the device: points (N, C) float32 CUDA, C >= 2, point_offsets
    (B + 1) on the HOST -> (out (4 N, C), out_offsets (4 B + 1) host int64, out_offsets_device): the batch of 4 B samples
    CenterHead.predict's double_flip expects, sample b's views at 4 b .. 4 b + 3: its rows as they are, with y = -y, with
    x = -x, with both (a sign-bit flip, as NumPy's unary minus). One enqueue (dal3_flip4_points), no synchronisation: the
    host offsets come from the host's, the device offsets from the kernel."""
    if not torch.is_tensor(points):
        raise TypeError("points must be a tensor")
    _hip.require_gpu(points, "points")
    if points.dim() != 2 or points.shape[1] < 2:
        raise ValueError(f"points must be (N, C >= 2), got {tuple(points.shape)}")
    if points.dtype != torch.float32:
        raise TypeError(f"points must be float32, got {points.dtype}")
    points = points.contiguous()
    N, C = points.shape
    off = _hip.host_offsets(point_offsets, N, "point_offsets", "the capacity of the outputs comes", "B")
    B, dev = off.size - 1, points.device
    n = np.diff(off)
    out_off = np.empty(4 * B + 1, np.int64)
    out_off[:-1] = (4 * off[:-1, None] + np.arange(4, dtype=np.int64)[None, :] * n[:, None]).reshape(-1)
    out_off[-1] = 4 * off[-1]
    off_dev = _device_ints(point_offsets_device, "point_offsets_device", torch.int64, B + 1, dev)
    if off_dev is None:
        off_dev = torch.from_numpy(off).to(dev)
    out = torch.empty((4 * N, C), dtype=torch.float32, device=dev)
    out_off_dev = torch.zeros(4 * B + 1, dtype=torch.int64, device=dev) if B == 0 else \
        torch.empty(4 * B + 1, dtype=torch.int64, device=dev)
    _hip.check(_hip.lib().dal3_flip4_points(_hip.ptr(points), N, C, _hip.ptr(off_dev), B, _hip.ptr(out), _hip.ptr(out_off_dev),
                                            int(max_workgroups), _hip.stream()))
    return out, out_off, out_off_dev


class VoxelGenerator:
    """det3d/core/input/voxel_generator.py: the reference's constructor and properties; `generate` takes one sample's
    points (a CUDA tensor) and returns its voxels, coordinates (M, 3) [z, y, x] and num_points as device tensors."""

    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000):
        self._point_cloud_range = np.array(point_cloud_range, dtype=np.float32)
        self._voxel_size = np.array(voxel_size, dtype=np.float32)
        self._grid_size = grid_size(self._voxel_size, self._point_cloud_range)
        self._max_num_points = max_num_points
        self._max_voxels = max_voxels

    def generate(self, points, max_voxels=-1):
        if max_voxels == -1:
            max_voxels = self._max_voxels
        r = voxelize(points, [0, points.shape[0]], self._voxel_size, self._point_cloud_range, self._max_num_points, max_voxels)
        voxels, coords, num, _ = r.finish()
        return voxels, coords[:, 1:], num

    @property
    def voxel_size(self):
        return self._voxel_size

    @property
    def max_num_points_per_voxel(self):
        return self._max_num_points

    @property
    def point_cloud_range(self):
        return self._point_cloud_range

    @property
    def grid_size(self):
        return self._grid_size


class PFNLayer(nn.Module):
    """One layer of the pillar feature net as a parameter container: `linear` (no bias) and `norm` (BatchNorm1d over the
    channels), the names a checkpoint uses. A middle layer has out_channels // 2 units: the other half of its output is
    the pillar's maximum repeated on every row. forward is stock torch (train mode, and the shapes the kernel does not
    serve)."""

    def __init__(self, in_channels, out_channels, norm_cfg=None, last_layer=False):
        super().__init__()
        cfg = dict(eps=1e-3, momentum=0.01) if norm_cfg is None else norm_cfg
        self.is_last = bool(last_layer)
        self.units = out_channels if self.is_last else out_channels // 2
        self.linear = nn.Linear(in_channels, self.units, bias=False)
        self.norm = nn.BatchNorm1d(self.units, eps=cfg.get("eps", 1e-5), momentum=cfg.get("momentum", 0.1))

    def forward(self, rows):
        """rows (P, T, c_in) -> (P, T, 2 * units), or (P, 1, units) from the last layer"""
        P, T = rows.shape[0], rows.shape[1]
        # every row of every pillar is one sample of the BatchNorm: (P * T, units), the statistics of (P, units, T)
        y = torch.relu(self.norm(self.linear(rows.reshape(P * T, -1)))).reshape(P, T, self.units)
        top = y.max(dim=1, keepdim=True).values
        return top if self.is_last else torch.cat([y, top.expand(P, T, self.units)], dim=2)


def _checked_voxels(features, num_voxels, coors):
    for t, what in ((features, "features"), (num_voxels, "num_voxels"), (coors, "coors")):
        if not torch.is_tensor(t):
            raise TypeError(f"{what} must be a tensor")
        _hip.require_gpu(t, what)
    if features.dim() != 3 or features.dtype != torch.float32:
        raise ValueError(f"features must be float32 (P, max_points, C), got {features.dtype} {tuple(features.shape)}")
    P = features.shape[0]
    if num_voxels.shape != (P,) or coors.shape != (P, 4):
        raise ValueError(f"num_voxels must be ({P},) and coors ({P}, 4), got {tuple(num_voxels.shape)}, {tuple(coors.shape)}")
    return features.contiguous(), num_voxels.to(torch.int32).contiguous(), coors.to(torch.int32).contiguous()


class PillarFeatureNet(nn.Module):
    """pillar_encoder.py:58-153. Eval mode with num_filters (64,) or (64, 64), with_distance=False, max_points <= 64 and
    3 .. 8 point features runs dal3_pillar_features (BatchNorm folded at packing time with the layers' own eps); anything
    else, and train mode, runs the stock-torch composite. forward -> (P, C_out) always (no squeeze). The training step on
    the HIP kernels is opt-in: `train_forward` / `train_forward_canvas` (dal3_pillar_train_forward / _backward)."""

    def __init__(self, num_input_features=4, num_filters=(64,), with_distance=False, voxel_size=(0.2, 0.2, 4),
                 pc_range=(0, -40, -3, 70.4, 40, 1), norm_cfg=None):
        super().__init__()
        if len(num_filters) < 1:
            raise ValueError("num_filters needs at least one layer")
        self.name = "PillarFeatureNet"
        self.num_input = int(num_input_features)
        self._with_distance = bool(with_distance)
        # a row is the point, its offset from the pillar's mean (3), from the pillar's centre (2) and, optionally, its range
        widths = [self.num_input + 5 + int(self._with_distance)] + [int(w) for w in num_filters]
        last = len(widths) - 2
        self.pfn_layers = nn.ModuleList(PFNLayer(widths[i], widths[i + 1], norm_cfg=norm_cfg, last_layer=i == last)
                                        for i in range(last + 1))
        # the centre of pillar (x, y) is coor * v + v / 2 + lo: the offsets are formed in double, as Python forms them
        self.vx, self.vy = voxel_size[0], voxel_size[1]
        self.x_offset, self.y_offset = self.vx / 2 + pc_range[0], self.vy / 2 + pc_range[1]
        self._packed, self._stamp = None, None

    # ------------------------------------------------------------------ the packed weights: a derived cache
    def invalidate_packed(self):
        """after writes that bypass the tensors' version counters (`.data` writes, raw pointers)"""
        self._packed, self._stamp = None, None

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self.invalidate_packed()
        return out

    def train(self, mode=True):
        out = super().train(mode)
        self.invalidate_packed()
        return out

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self.invalidate_packed()
        return out

    def _tensors(self):
        return [t for l in self.pfn_layers
                for t in (l.linear.weight, l.norm.weight, l.norm.bias, l.norm.running_mean, l.norm.running_var)]

    def hip_serves(self, max_points=20):
        """whether the eval-mode forward of this module runs the HIP kernel"""
        units = [l.units for l in self.pfn_layers]
        eps = {l.norm.eps for l in self.pfn_layers}
        return (not self._with_distance and units in ([64], [32, 64]) and 3 <= self.num_input <= 8 and len(eps) == 1
                and 1 <= max_points <= 64 and all(l.norm.affine and l.norm.track_running_stats for l in self.pfn_layers))

    def packed(self):
        ts = self._tensors()
        stamp = tuple((t.data_ptr(), t._version, t.device) for t in ts)
        if self._packed is None or stamp != self._stamp:
            # (only the check is shared with the MFMA layers' packers: dal3_pillar_pack folds with its own kernel)
            layers = (_hip.Layer * len(self.pfn_layers))(*[_hip.fold_layer_struct(l.linear, l.norm, "PillarFeatureNet's parameters")
                                                           for l in self.pfn_layers])
            buf = torch.empty(_hip.PILLAR_PACK_FLOATS, dtype=torch.float32, device=ts[0].device)
            _hip.check(_hip.lib().dal3_pillar_pack(layers, len(self.pfn_layers), self.num_input,
                                                   float(self.pfn_layers[0].norm.eps), _hip.ptr(buf), _hip.stream()))
            self._packed, self._stamp = buf, stamp
        return self._packed

    def _launch(self, features, num_voxels, coors, n_pillars=None, canvas=None):
        P, max_points, C = features.shape
        out = None if canvas is not None else torch.empty((P, 64), dtype=torch.float32, device=features.device)
        a = _hip.PillarFeatureArgs(P=P, n_pillars=_hip.ptr(n_pillars), voxels=_hip.ptr(features), num_points=_hip.ptr(num_voxels),
                                   coordinates=_hip.ptr(coors), C=C, max_points=max_points, n_layers=len(self.pfn_layers),
                                   c_out=64, vx=self.vx, vy=self.vy, x_offset=self.x_offset, y_offset=self.y_offset,
                                   packed=_hip.ptr(self.packed()), features=_hip.ptr(out), canvas=_hip.ptr(canvas))
        if canvas is not None:
            a.canvas_B, a.ny, a.nx = canvas.shape[0], canvas.shape[2], canvas.shape[3]
        _hip.check(_hip.lib().dal3_pillar_features(a, _hip.stream()))
        return canvas if canvas is not None else out

    def composite(self, features, num_voxels, coors):
        """the same definition (include/dal3.h, dal3_pillar_features) in stock torch ops -> (P, C_out); differentiable, and in
        train mode the BatchNorms use and update their batch statistics"""
        P, T = features.shape[0], features.shape[1]
        xyz = features[..., :3]
        mean = xyz.sum(dim=1, keepdim=True) / num_voxels.to(features.dtype).reshape(P, 1, 1)
        centre = coors[:, [3, 2]].to(features.dtype) * features.new_tensor([self.vx, self.vy]) + \
            features.new_tensor([self.x_offset, self.y_offset])
        parts = [features, xyz - mean, features[..., :2] - centre.reshape(P, 1, 2)]
        if self._with_distance:
            parts.append(torch.linalg.vector_norm(xyz, dim=2, keepdim=True))
        real = torch.arange(T, device=features.device).reshape(1, T) < num_voxels.reshape(P, 1)
        rows = torch.cat(parts, dim=2) * real.reshape(P, T, 1).to(features.dtype)
        for layer in self.pfn_layers:
            rows = layer(rows)
        return rows.reshape(P, -1)


    def forward(self, features, num_voxels, coors):
        if self.training or features.dim() != 3 or features.shape[2] != self.num_input or not self.hip_serves(features.shape[1]):
            return self.composite(features, num_voxels, coors)
        with torch.no_grad():
            return self._launch(*_checked_voxels(features, num_voxels, coors))

    @torch.no_grad()
    def forward_canvas(self, features, num_voxels, coors, batch_size, input_shape, n_pillars=None):
        """the fused route: features -> the (batch_size, 64, ny, nx) canvas directly, the (P, 64) tensor never exists;
        input_shape = [nx, ny, ...] as PointPillarsScatter takes it. The bits of forward + PointPillarsScatter."""
        if self.training or not self.hip_serves(features.shape[1]) or features.shape[2] != self.num_input:
            raise RuntimeError("the fused route needs the module in eval mode and a shape the HIP kernel serves (hip_serves)")
        features, num_voxels, coors = _checked_voxels(features, num_voxels, coors)
        n_pillars = _device_ints(n_pillars, "n_pillars", torch.int64, 1, features.device)
        canvas = torch.empty((int(batch_size), 64, int(input_shape[1]), int(input_shape[0])), dtype=torch.float32,
                             device=features.device)
        return self._launch(features, num_voxels, coors, n_pillars, canvas)

    # ------------------------------------------------------------------ the training step (dal3_pillar_train_*)
    def _train_checked(self, features, num_voxels, coors, n_pillars, route):
        if not self.training:
            raise RuntimeError(f"PillarFeatureNet.{route} is the training step: the module is in eval mode (call .train(); "
                               "forward / forward_canvas serve eval mode)")
        if features.dim() != 3 or features.shape[2] != self.num_input or not self.hip_serves(features.shape[1]):
            raise RuntimeError(f"PillarFeatureNet.{route}: hip_serves does not serve this shape (units [64] or [32, 64], "
                               f"3 <= C <= 8, max_points <= 64, one eps, with_distance=False); got units "
                               f"{[l.units for l in self.pfn_layers]}, features {tuple(features.shape)}, "
                               f"num_input_features {self.num_input}, with_distance {self._with_distance}")
        features, num_voxels, coors = _checked_voxels(features, num_voxels, coors)
        if features.shape[0] * features.shape[1] < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                             f"{[features.shape[0] * features.shape[1], self.pfn_layers[0].units]}")
        for t in self._tensors():
            _hip.require_gpu(t, "PillarFeatureNet's parameters")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("weights must be contiguous fp32")
        return features, num_voxels, coors, _device_ints(n_pillars, "n_pillars", torch.int64, 1, features.device)

    def train_forward(self, features, num_voxels, coors, n_pillars=None, *, max_workgroups=0):
        """train mode on the HIP kernels -> (P, 64), differentiable with respect to every linear.weight, norm.weight and
        norm.bias (not the voxels). The BatchNorms use the batch statistics of the first min(*n_pillars, P) pillars' rows
        and update running_mean / running_var / num_batches_tracked in place, on the device; rows behind the live count
        are zero and nothing of them is read. No host synchronisation."""
        features, num_voxels, coors, n_pillars = self._train_checked(features, num_voxels, coors, n_pillars, "train_forward")
        params = [t for l in self.pfn_layers for t in (l.linear.weight, l.norm.weight, l.norm.bias)]
        return _PillarTrain.apply(self, features, num_voxels, coors, n_pillars, None, int(max_workgroups), *params)

    def train_forward_canvas(self, features, num_voxels, coors, batch_size, input_shape, n_pillars=None, *, max_workgroups=0):
        """the fused training route -> the differentiable (batch_size, 64, ny, nx) canvas, the bits of train_forward +
        PointPillarsScatter; the backward reads the canvas cotangent through its strides, the (P, 64) tensors never exist.
        input_shape = [nx, ny, ...]."""
        features, num_voxels, coors, n_pillars = self._train_checked(features, num_voxels, coors, n_pillars, "train_forward_canvas")
        params = [t for l in self.pfn_layers for t in (l.linear.weight, l.norm.weight, l.norm.bias)]
        shape = (int(batch_size), 64, int(input_shape[1]), int(input_shape[0]))
        return _PillarTrain.apply(self, features, num_voxels, coors, n_pillars, shape, int(max_workgroups), *params)

    def _train_args(self, features, num_voxels, coors, n_pillars, params, saved, ws, max_workgroups):
        P, max_points, C = features.shape
        layers = (_hip.Layer * len(self.pfn_layers))(*[
            _hip.Layer(_hip.ptr(params[3 * i]), None, _hip.ptr(params[3 * i + 1]), _hip.ptr(params[3 * i + 2]), None, None,
                       params[3 * i].shape[1], params[3 * i].shape[0]) for i in range(len(self.pfn_layers))])
        a = _hip.PillarTrainArgs(P=P, n_pillars=_hip.ptr(n_pillars), voxels=_hip.ptr(features), num_points=_hip.ptr(num_voxels),
                                 coordinates=_hip.ptr(coors), C=C, max_points=max_points, n_layers=len(self.pfn_layers), c_out=64,
                                 vx=self.vx, vy=self.vy, x_offset=self.x_offset, y_offset=self.y_offset, layers=layers,
                                 eps=float(self.pfn_layers[0].norm.eps), saved=_hip.ptr(saved), max_workgroups=max_workgroups,
                                 workspace=_hip.ptr(ws), workspace_bytes=ws.numel())
        return a, layers                # (the caller keeps `layers` alive over the call)


class _PillarTrain(torch.autograd.Function):
    """dal3_pillar_train_forward / dal3_pillar_train_backward: params = (linear.weight, norm.weight, norm.bias) per layer"""

    @staticmethod
    def forward(ctx, net, features, num_voxels, coors, n_pillars, canvas_shape, max_workgroups, *params):
        dev = features.device
        params = [p.detach() for p in params]
        lib = _hip.lib()
        ws = _hip.workspace(lib.dal3_pillar_train_workspace_bytes(features.shape[0], len(net.pfn_layers)), dev)
        saved = torch.empty(_hip.PILLAR_TRAIN_SAVED_FLOATS, dtype=torch.float32, device=dev)
        a, keep = net._train_args(features, num_voxels, coors, n_pillars, params, saved, ws, max_workgroups)
        for i, l in enumerate(net.pfn_layers):
            # momentum None is torch's cumulative average: not what the reference's configs use, and not served
            if l.norm.momentum is None:
                raise RuntimeError("PillarFeatureNet.train_forward: BatchNorm momentum=None (a cumulative average) is not served")
            a.momentum[i] = float(l.norm.momentum)
            a.running_mean[i], a.running_var[i] = l.norm.running_mean.data_ptr(), l.norm.running_var.data_ptr()
            a.num_batches_tracked[i] = l.norm.num_batches_tracked.data_ptr()
        if canvas_shape is None:
            out = torch.empty((features.shape[0], 64), dtype=torch.float32, device=dev)
            a.features = out.data_ptr()
        else:
            out = torch.empty(canvas_shape, dtype=torch.float32, device=dev)
            a.canvas, a.canvas_B, a.ny, a.nx = out.data_ptr(), canvas_shape[0], canvas_shape[2], canvas_shape[3]
        _hip.check(lib.dal3_pillar_train_forward(a, _hip.stream()))
        net.invalidate_packed()         # the kernels wrote the running statistics through raw pointers
        ctx.net, ctx.canvas_shape, ctx.max_workgroups, ctx.n_pillars = net, canvas_shape, max_workgroups, n_pillars
        ctx.save_for_backward(features, num_voxels, coors, saved, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        features, num_voxels, coors, saved, *params = ctx.saved_tensors
        net, dev = ctx.net, features.device
        lib = _hip.lib()
        if grad.dtype != torch.float32:
            raise TypeError(f"PillarFeatureNet.train_forward: the cotangent must be float32, got {grad.dtype}")
        ws = _hip.workspace(lib.dal3_pillar_train_workspace_bytes(features.shape[0], len(net.pfn_layers)), dev)
        a, keep = net._train_args(features, num_voxels, coors, ctx.n_pillars, params, saved, ws, ctx.max_workgroups)
        a.grad = grad.data_ptr()
        if ctx.canvas_shape is None:
            a.grad_stride[:] = [grad.stride(0), grad.stride(1), 0, 0]
        else:
            a.canvas = grad.data_ptr()
            a.canvas_B, a.ny, a.nx = ctx.canvas_shape[0], ctx.canvas_shape[2], ctx.canvas_shape[3]
            a.grad_stride[:] = list(grad.stride())
        grads = [torch.empty_like(p) for p in params]
        for i in range(len(net.pfn_layers)):
            a.dW[i], a.dgamma[i], a.dbeta[i] = (g.data_ptr() for g in grads[3 * i:3 * i + 3])
        _hip.check(lib.dal3_pillar_train_backward(a, _hip.stream()))
        return (None,) * 7 + tuple(grads)


class PointPillarsScatter(nn.Module):
    """pillar_encoder.py:156-209 as dal3_pillar_scatter: one launch for the batch, cells are unique per sample"""

    def __init__(self, num_input_features=64, norm_cfg=None, name="PointPillarsScatter", **kwargs):
        super().__init__()
        self.name = "PointPillarsScatter"
        self.nchannels = num_input_features

    @torch.no_grad()
    def forward(self, voxel_features, coords, batch_size, input_shape, n_pillars=None):
        self.nx = input_shape[0]
        self.ny = input_shape[1]
        for t, what in ((voxel_features, "voxel_features"), (coords, "coords")):
            if not torch.is_tensor(t):
                raise TypeError(f"{what} must be a tensor")
            _hip.require_gpu(t, what)
        P = voxel_features.shape[0]
        if voxel_features.dim() != 2 or voxel_features.shape[1] != self.nchannels or voxel_features.dtype != torch.float32:
            raise ValueError(f"voxel_features must be float32 (P, {self.nchannels}), got {tuple(voxel_features.shape)}")
        if coords.shape != (P, 4):
            raise ValueError(f"coords must be ({P}, 4), got {tuple(coords.shape)}")
        voxel_features, coords = voxel_features.contiguous(), coords.to(torch.int32).contiguous()
        n_pillars = _device_ints(n_pillars, "n_pillars", torch.int64, 1, voxel_features.device)
        canvas = torch.empty((int(batch_size), self.nchannels, int(self.ny), int(self.nx)), dtype=torch.float32,
                             device=voxel_features.device)
        _hip.check(_hip.lib().dal3_pillar_scatter(_hip.ptr(voxel_features), _hip.ptr(coords), P, _hip.ptr(n_pillars), self.nchannels,
                                                  _hip.ptr(canvas), int(batch_size), int(self.ny), int(self.nx), _hip.stream()))
        return canvas


class VoxelFeatureExtractorV3(nn.Module):
    """voxel_encoder.py:9-24 as dal3_voxel_mean: the sum over a voxel's rows / num_points -> (P, C)"""

    def __init__(self, num_input_features=4, norm_cfg=None, name="VoxelFeatureExtractorV3"):
        super().__init__()
        self.name = name
        self.num_input_features = num_input_features

    @torch.no_grad()
    def forward(self, features, num_voxels, coors=None, n_pillars=None):
        assert self.num_input_features == features.shape[-1]
        for t, what in ((features, "features"), (num_voxels, "num_voxels")):
            _hip.require_gpu(t, what)
        if features.dim() != 3 or features.dtype != torch.float32 or num_voxels.shape != (features.shape[0],):
            raise ValueError("features must be float32 (P, max_points, C) and num_voxels (P,)")
        features, num_voxels = features.contiguous(), num_voxels.to(torch.int32).contiguous()
        n_pillars = _device_ints(n_pillars, "n_pillars", torch.int64, 1, features.device)
        P, T, C = features.shape
        out = torch.empty((P, C), dtype=torch.float32, device=features.device)
        _hip.check(_hip.lib().dal3_voxel_mean(_hip.ptr(features), _hip.ptr(num_voxels), P, _hip.ptr(n_pillars), T, C, _hip.ptr(out),
                                              _hip.stream()))
        return out


class PillarReader(nn.Module):
    """points + offsets -> the BEV canvas: voxelise -> pillar features -> scatter, enqueued on the current stream with no
    host synchronisation. cfg (a dict): voxel_size, pc_range, max_points, max_voxels, num_input_features, and optionally
    num_filters (default (64, 64)) and norm_cfg. The canvas is (B, 64, ny, nx); `last` keeps the VoxelizeResult."""

    def __init__(self, cfg):
        super().__init__()
        self.voxel_size = [float(v) for v in cfg["voxel_size"]]
        self.pc_range = [float(v) for v in cfg["pc_range"]]
        self.max_points, self.max_voxels = int(cfg["max_points"]), int(cfg["max_voxels"])
        self.grid = grid_size(self.voxel_size, self.pc_range)
        self.reader = PillarFeatureNet(num_input_features=int(cfg["num_input_features"]),
                                       num_filters=tuple(cfg.get("num_filters", (64, 64))), voxel_size=self.voxel_size,
                                       pc_range=self.pc_range, norm_cfg=cfg.get("norm_cfg"))
        self.last = None

    @torch.no_grad()
    def forward(self, points, point_offsets, allocator=None, point_offsets_device=None):
        """point_offsets on the HOST (the output sizes come from it); point_offsets_device: the same values as a CUDA int64
        tensor. Without it the B + 1 offsets are uploaded from pageable memory on every call, the one host-to-device
        copy of this route."""
        if self.training:
            raise RuntimeError("PillarReader is the eval-mode route: call .eval()")
        r = voxelize(points, point_offsets, self.voxel_size, self.pc_range, self.max_points, self.max_voxels, allocator=allocator,
                     point_offsets_device=point_offsets_device)
        self.last = r
        return self.reader.forward_canvas(r.voxels, r.num_points, r.coordinates, r.B, [int(self.grid[0]), int(self.grid[1])],
                                          n_pillars=r.n_pillars)
