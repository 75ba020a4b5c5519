"""CenterPoint's one-stage detectors, eval mode, on the GPU: `PointPillars` (det3d/models/detectors/point_pillars.py,
single_stage.py) and `VoxelNet` (det3d/models/detectors/voxelnet.py) under the reference's names, constructor signatures
and state_dict keys (`reader.*`, `backbone.*`, `neck.*`, `bbox_head.*`; the scatter backbone and the voxel-mean reader have
no parameters), built from the `model` dict of a config such as configs/waymo/pp/waymo_centerpoint_pp_two_pfn_stride1_3x.py
or configs/waymo/voxelnet/waymo_centerpoint_voxelnet_3x.py.

`forward(example, return_loss=False)` takes the reference's collated example (voxels, coordinates, num_points, num_voxels,
shape, metadata) and returns `CenterHead.predict`'s list. `detect(points, point_offsets, metadata=None)` starts from the
raw sweep instead: voxelise -> pillar features into the canvas -> RPN -> CenterHead -> decode + NMS, everything enqueued on
the current stream; the read-back of the kept boxes inside `predict` is the only host synchronisation. `PointPillars.
first_stage_loss(example, reader="hip")` and `train_step_from_sweeps` are its training step up to the loss, the reader on
its HIP training kernels. A `test_cfg` with
`double_flip` (test-time augmentation) is served by both: `forward` takes the reference's batch of four views per sample,
`detect` makes the views itself. Only `forward(return_loss=True)` is refused: the loss is reached through
`first_stage_loss`, not through `forward`. `VoxelNet` has the same two doors
with the 3-D grid, VoxelFeatureExtractorV3 and the sparse middle (sparse.SpMiddleResNetFHD) in front of the neck.
`VoxelNet.first_stage_loss(example)` is the training step up to the loss: the reader, the backbone's differentiable
`train_forward`, the neck's and the head's stock-torch routes (or, with `dense="hip"`, their `train_forward` on the HIP
convolution kernels) and `CenterHead.loss` (`forward(return_loss=True)` stays refused). `forward_two_stage` stays refused: the two-stage model is two_stage.TwoStageDetector, which wraps either detector, runs
its stages up to the head itself and keeps the kept boxes on the device for the RoI head.
"""
import torch
from torch import nn

from . import pillars, rpn, sparse
from .detect import CenterHeadPost, _get

READERS = {"PillarFeatureNet": pillars.PillarFeatureNet, "VoxelFeatureExtractorV3": pillars.VoxelFeatureExtractorV3}
BACKBONES = {"PointPillarsScatter": pillars.PointPillarsScatter, "SpMiddleResNetFHD": sparse.SpMiddleResNetFHD}
NECKS = {"RPN": rpn.RPN}
HEADS = {"CenterHead": rpn.CenterHead}
DENSE_ROUTES = ("composite", "hip")             # how the neck and the head train (first_stage_loss)
READER_ROUTES = ("composite", "hip")            # how the pillar reader trains (PointPillars.first_stage_loss)


def _build(cfg, table, what):
    if isinstance(cfg, nn.Module):
        return cfg
    args = dict(cfg)
    kind = args.pop("type")
    if kind not in table:
        raise KeyError(f"{what} type {kind!r} is not built here (known: {sorted(table)})")
    return table[kind](**args)


class SingleStageDetector(nn.Module):
    """what the one-stage detectors share (det3d/models/detectors/single_stage.py): the four stages built from the config's
    dicts (with `type`) or given as modules, the checkpoint door, and the start of `detect`."""

    def __init__(self, reader, backbone, neck, bbox_head, train_cfg, test_cfg, max_points, max_voxels, voxel_size, pc_range):
        super().__init__()
        self.reader = _build(reader, READERS, "reader")
        self.backbone = _build(backbone, BACKBONES, "backbone")
        self.neck = _build(neck, NECKS, "neck")
        self.bbox_head = _build(bbox_head, HEADS, "bbox_head")
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.max_points, self.max_voxels = int(max_points), int(max_voxels)
        self.voxel_size, self.pc_range = voxel_size, pc_range
        self.last = None

    @property
    def with_neck(self):
        return self.neck is not None

    @property
    def precision(self):
        """the MFMA operand type of the dense stage's eval-mode kernels: 'fp32' (the default) | 'fp16' | 'bf16'. Setting it
        sets the neck's and the head's `precision` (rpn.RPN, rpn.CenterHead), whose maps stay float32 either way. The reader
        (PillarFeatureNet / the voxel mean) and the sparse 3-D middle stay fp32, and so do the decode and the NMS."""
        return self.bbox_head.precision

    @precision.setter
    def precision(self, value):
        rpn.check_precision(value)
        for m in (self.neck, self.bbox_head):
            if m is not None:
                m.precision = value

    @property
    def sparse_precision(self):
        """the MFMA operand type of the sparse 3-D middle's eval-mode convolutions (sparse.SpMiddleResNetFHD.sparse_precision):
        'fp32' (the default) | 'fp16' | 'bf16'. A knob of its own: `precision` does not touch it, and it does not touch
        `precision`. A backbone without one (PointPillarsScatter) reads 'fp32' and refuses to be set."""
        return getattr(self.backbone, "sparse_precision", "fp32")

    @sparse_precision.setter
    def sparse_precision(self, value):
        rpn.check_precision(value)
        if not hasattr(self.backbone, "sparse_precision"):
            raise ValueError(f"{type(self.backbone).__name__} has no sparse convolutions: sparse_precision belongs to a detector "
                             "with a sparse 3-D middle (VoxelNet)")
        self.backbone.sparse_precision = value

    def init_weights(self, pretrained):
        """a checkpoint path: its `state_dict` (or the file itself) must hold exactly this model's keys"""
        ckpt = torch.load(pretrained, map_location="cpu")
        self.load_state_dict(ckpt.get("state_dict", ckpt), strict=True)

    def _refuse_loss(self, return_loss):
        if return_loss:
            raise NotImplementedError(f"{type(self).__name__}.forward(return_loss=True): the detector's loss is not built; this is "
                                      "the eval-mode detector (call with return_loss=False)")

    def _voxelize(self, points, point_offsets, point_offsets_device):
        """the start of `detect`: the checks, the four flipped views of test_cfg.double_flip, the voxelisation (kept in `last`)"""
        if self.training:
            raise RuntimeError("detect is the eval-mode route: call .eval()")
        if self.voxel_size is None:
            raise RuntimeError("detect needs the reader's voxel_size and pc_range: build the model from the config's dicts")
        if _get(self.test_cfg, "double_flip", False):
            # four views per sample (the sweep, y = -y, x = -x, both), merged again by DoubleFlipPost inside predict
            points, point_offsets, point_offsets_device = pillars.double_flip(points, point_offsets, point_offsets_device)
        r = pillars.voxelize(points, point_offsets, self.voxel_size, self.pc_range, self.max_points, self.max_voxels,
                             point_offsets_device=point_offsets_device)
        self.last = r
        return r

    def set_train_input(self, preprocess, assigner):
        """the stages `train_step_from_sweeps` feeds the loss with: an augment.Preprocess and a center_loss.AssignLabel"""
        self.train_input = (preprocess, assigner)

    def _example_from_sweeps(self, points, point_offsets, annotations, draws):
        """augment.train_example on this detector's grid: the capacity-sized example of `train_step_from_sweeps`"""
        if getattr(self, "train_input", None) is None:
            raise RuntimeError("train_step_from_sweeps needs set_train_input(preprocess, assigner) first")
        if self.voxel_size is None:
            raise RuntimeError("train_step_from_sweeps needs the reader's voxel_size and pc_range: build the model with them")
        from . import augment
        preprocess, assigner = self.train_input
        return augment.train_example(preprocess, assigner, points, point_offsets, annotations["gt_boxes"], annotations["gt_classes"],
                                     annotations["gt_counts"], voxel_size=self.voxel_size, pc_range=self.pc_range,
                                     max_points=self.max_points, max_voxels=self.max_voxels, draws=draws,
                                     candidates=annotations.get("candidates"))

    to_prediction = staticmethod(CenterHeadPost.to_prediction)


class PointPillars(SingleStageDetector):
    """reader / backbone / neck / bbox_head: the config's dicts (with `type`) or modules. max_points / max_voxels: the
    config's voxel_generator (max_points_in_voxel, max_voxel_num), which `detect` voxelises with."""

    def __init__(self, reader, backbone, neck, bbox_head, train_cfg=None, test_cfg=None, pretrained=None, *, max_points=20,
                 max_voxels=60000):
        super().__init__(reader, backbone, neck, bbox_head, train_cfg, test_cfg, max_points, max_voxels, None, None)
        if isinstance(reader, dict):
            self.voxel_size, self.pc_range = list(reader["voxel_size"]), list(reader["pc_range"])
        if pretrained is not None:
            self.init_weights(pretrained)

    def extract_feat(self, data):
        features = self.reader(data["features"], data["num_voxels"], data["coors"])
        x = self.backbone(features, data["coors"], data["batch_size"], data["input_shape"])
        return self.neck(x) if self.with_neck else x

    def forward(self, example, return_loss=False, **kwargs):
        self._refuse_loss(return_loss)
        data = dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"],
                    batch_size=len(example["num_voxels"]), input_shape=example["shape"][0])
        preds = self.bbox_head(self.extract_feat(data))
        return self.bbox_head.predict(example, preds, self.test_cfg)

    def first_stage_loss(self, example, reader="hip", dense="composite"):
        """the training step up to the loss: reader -> canvas -> the neck and the head (BatchNorm by its mode) ->
        CenterHead.loss. reader: "hip" (the default: PillarFeatureNet.train_forward_canvas, the reader's forward and
        backward on the HIP kernels; it honours example["n_voxels"], the device count of a capacity-sized batch) |
        "composite" (stock torch ops, stock autograd and an index_put scatter). dense: the neck's and the head's route, as
        VoxelNet.first_stage_loss takes it. example: the voxeliser's entries (voxels, coordinates, num_points, num_voxels,
        shape; optionally n_voxels) and the lists of center_loss.center_targets -> CenterHead.loss's dictionary; `loss`
        carries the graph to every parameter of the reader, the neck and the head."""
        if reader not in READER_ROUTES:
            raise ValueError(f"reader {reader!r}: the pillar reader trains through 'hip' (its kernels) or 'composite' (stock torch)")
        if dense not in DENSE_ROUTES:
            raise ValueError(f"dense {dense!r}: the neck and the head train through 'composite' (stock torch) or 'hip'")
        n_voxels, B, shape = example.get("n_voxels"), len(example["num_voxels"]), example["shape"][0]
        voxels, num, co = example["voxels"], example["num_points"], example["coordinates"]
        if reader == "hip":
            x = self.reader.train_forward_canvas(voxels, num, co, B, shape, n_pillars=n_voxels)
        else:
            if n_voxels is not None:
                raise ValueError("reader='composite' cannot take a capacity-sized batch (n_voxels): the rows behind the live count "
                                 "have num_points 0, the composite divides by it, and the 0 / 0 = NaN goes into BatchNorm's batch "
                                 "statistics. Slice the example to its live rows and drop n_voxels (a host read-back), or use "
                                 "reader='hip'")
            feats = self.reader.composite(voxels, num, co)
            at = co.long()
            x = feats.new_zeros((B, feats.shape[1], int(shape[1]), int(shape[0])))
            x[at[:, 0], :, at[:, 2], at[:, 3]] = feats
        hip = dense == "hip"
        if self.with_neck:
            x = self.neck.train_forward(x) if hip else self.neck.composite(x)
        return self.bbox_head.loss(example, self.bbox_head.train_forward(x) if hip else self.bbox_head.composite(x))

    def train_step_from_sweeps(self, points, point_offsets, annotations, draws=None, reader="hip", dense="composite"):
        """VoxelNet.train_step_from_sweeps's contract on the pillar grid: resident sweeps and annotations ->
        CenterHead.loss's dictionary on the current stream with no host synchronisation (augment.train_example, then
        first_stage_loss with `reader` and `dense`). `last_example` keeps the example."""
        self.last_example = self._example_from_sweeps(points, point_offsets, annotations, draws)
        return self.first_stage_loss(self.last_example, reader=reader, dense=dense)

    @torch.no_grad()
    def detect(self, points, point_offsets, metadata=None, point_offsets_device=None):
        """points (N, C) float32 CUDA, point_offsets (B + 1) on the host -> the per-sample list of box3d_lidar / scores /
        label_preds / metadata (CenterHeadPost.to_prediction turns it into the prediction.pkl dictionary). `last` keeps the
        VoxelizeResult. With test_cfg.double_flip the sweep is first copied into its four flipped views (pillars.double_flip),
        everything up to the head runs on 4 B samples (`last` is theirs) and the post-processing merges them into B."""
        r = self._voxelize(points, point_offsets, point_offsets_device)
        grid = pillars.grid_size(self.voxel_size, self.pc_range)
        canvas = self.reader.forward_canvas(r.voxels, r.num_points, r.coordinates, r.B, [int(grid[0]), int(grid[1])],
                                            n_pillars=r.n_pillars)
        preds = self.bbox_head(self.neck(canvas))
        return self.bbox_head.predict({"metadata": metadata}, preds, self.test_cfg)


class VoxelNet(SingleStageDetector):
    """det3d/models/detectors/voxelnet.py, one stage: VoxelFeatureExtractorV3 -> SpMiddleResNetFHD -> RPN -> CenterHead.
    max_points / max_voxels / voxel_size / pc_range: the config's voxel_generator (max_points_in_voxel, max_voxel_num,
    voxel_size, range), which `detect` voxelises with on the 3-D grid. sparse_capacities: the rows of the backbone's
    strided levels ({"conv2": ..}, see sparse.SpMiddleResNetFHD; None: the safe bounds)."""

    def __init__(self, reader, backbone, neck, bbox_head, train_cfg=None, test_cfg=None, pretrained=None, *, max_points=5,
                 max_voxels=150000, voxel_size=None, pc_range=None, sparse_capacities=None):
        super().__init__(reader, backbone, neck, bbox_head, train_cfg, test_cfg, max_points, max_voxels,
                         None if voxel_size is None else list(voxel_size), None if pc_range is None else list(pc_range))
        self.sparse_capacities = sparse_capacities
        if pretrained is not None:
            self.init_weights(pretrained)

    def extract_feat(self, data, n_voxels=None):
        """-> (x, voxel_feature): the neck's map and the backbone's {conv1 .. conv4} sparse tensors"""
        input_features = self.reader(data["features"], data["num_voxels"], n_pillars=n_voxels)
        x, voxel_feature = self.backbone(input_features, data["coors"], data["batch_size"], data["input_shape"],
                                         n_voxels=n_voxels, capacities=self.sparse_capacities)
        if self.with_neck:
            x = self.neck(x)
        return x, voxel_feature

    def forward(self, example, return_loss=False, **kwargs):
        self._refuse_loss(return_loss)
        data = dict(features=example["voxels"], num_voxels=example["num_points"], coors=example["coordinates"],
                    batch_size=len(example["num_voxels"]), input_shape=example["shape"][0])
        x, _ = self.extract_feat(data)
        return self.bbox_head.predict(example, self.bbox_head(x), self.test_cfg)

    def first_stage_loss(self, example, dense="composite"):
        """the first stage's training step up to its loss: reader -> backbone.train_forward -> the neck and the head
        (BatchNorm by its mode) -> CenterHead.loss. dense: the neck's and the head's route, "composite" (the default:
        stock torch ops and stock autograd) | "hip" (their `train_forward`: every convolution and its backward on the HIP
        kernels, float32 whatever `precision` says). example: the voxeliser's entries (voxels, coordinates, num_points,
        num_voxels, shape; optionally n_voxels, the device count of a capacity-sized batch) and the lists of
        center_loss.center_targets -> CenterHead.loss's dictionary; `loss` carries the graph to every parameter of the
        backbone, the neck and the head."""
        if dense not in DENSE_ROUTES:
            raise ValueError(f"dense {dense!r}: the neck and the head train through 'composite' (stock torch) or 'hip'")
        n_voxels = example.get("n_voxels")
        feats = self.reader(example["voxels"], example["num_points"], n_pillars=n_voxels)
        x, _ = self.backbone.train_forward(feats, example["coordinates"], len(example["num_voxels"]), example["shape"][0],
                                           n_voxels=n_voxels, capacities=self.sparse_capacities)
        hip = dense == "hip"
        if self.with_neck:
            x = self.neck.train_forward(x) if hip else self.neck.composite(x)
        return self.bbox_head.loss(example, self.bbox_head.train_forward(x) if hip else self.bbox_head.composite(x))

    def train_step_from_sweeps(self, points, point_offsets, annotations, draws=None, dense="composite"):
        """resident sweeps and annotations -> CenterHead.loss's dictionary, on the current stream with no host
        synchronisation: augment.train_example (GT paste, augmentation, shuffle; voxelisation; AssignLabel) and then
        first_stage_loss (`dense`: its route for the neck and the head). points (N, F) float32 CUDA, point_offsets (B + 1) on the host, annotations: {gt_boxes (B, max_gt, 9)
        CUDA, gt_classes, gt_counts} as augment.Preprocess takes them; draws: the step's augment.Draws (None: drawn on the
        device). `last_example` keeps the example."""
        example = self._example_from_sweeps(points, point_offsets, annotations, draws)
        self.last_example = example
        return self.first_stage_loss(example, dense=dense)

    def forward_two_stage(self, example, return_loss=False, **kwargs):
        raise NotImplementedError("VoxelNet.forward_two_stage: the second stage is not built into this method: two_stage."
                                  "TwoStageDetector runs the first stage through extract_feat and bbox_head itself")

    @torch.no_grad()
    def detect(self, points, point_offsets, metadata=None, point_offsets_device=None):
        """PointPillars.detect's contract on the 3-D grid: voxelise -> voxel mean -> sparse backbone -> RPN -> CenterHead ->
        decode + NMS on the current stream; the read-back inside `predict` is the only host synchronisation. `last` keeps the
        VoxelizeResult; the backbone's `last_status` holds the sparse levels' status word."""
        r = self._voxelize(points, point_offsets, point_offsets_device)
        grid = pillars.grid_size(self.voxel_size, self.pc_range)
        data = dict(features=r.voxels, num_voxels=r.num_points, coors=r.coordinates, batch_size=r.B,
                    input_shape=[int(g) for g in grid])
        x, _ = self.extract_feat(data, n_voxels=r.n_pillars)
        return self.bbox_head.predict({"metadata": metadata}, self.bbox_head(x), self.test_cfg)
