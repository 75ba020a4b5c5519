"""3dal_pytorch_amd/config.py and the host side of 3dal_pytorch_amd/waymo.py without a GPU: a config file in the reference's
format, written by the test itself (a two-stage model over VoxelNet at reduced neck widths), through Config.fromfile,
WaymoDataset's reading of the pipeline, build_detector and load_checkpoint."""
import importlib
import os
import pickle
import sys
from collections import OrderedDict

import pytest
import torch

config = importlib.import_module("3dal_pytorch_amd.config")
waymo = importlib.import_module("3dal_pytorch_amd.waymo")
two_stage = importlib.import_module("3dal_pytorch_amd.two_stage")
detector = importlib.import_module("3dal_pytorch_amd.detector")

TEXT = '''
import itertools
import logging

from det3d.utils.config_tool import get_downsample_factor

tasks = [
    dict(num_class=3, class_names=['VEHICLE', 'PEDESTRIAN', 'CYCLIST']),
]
class_names = list(itertools.chain(*[t["class_names"] for t in tasks]))
target_assigner = dict(tasks=tasks)

model = dict(
    type='TwoStageDetector',
    first_stage_cfg=dict(
        type="VoxelNet",
        pretrained='work_dirs/not_there/epoch_36.pth',
        reader=dict(type="VoxelFeatureExtractorV3", num_input_features=6),
        backbone=dict(type="SpMiddleResNetFHD", num_input_features=6, ds_factor=8),
        neck=dict(
            type="RPN",
            layer_nums=[5, 5],
            ds_layer_strides=[1, 2],
            ds_num_filters=[32, 64],
            us_layer_strides=[1, 2],
            us_num_filters=[64, 64],
            num_input_features=256,
            logger=logging.getLogger("RPN"),
        ),
        bbox_head=dict(
            type="CenterHead",
            in_channels=sum([64, 64]),
            tasks=tasks,
            dataset='waymo',
            weight=2,
            code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0],
            common_heads={'reg': (2, 2), 'height': (1, 2), 'dim': (3, 2), 'rot': (2, 2), 'vel': (2, 2)},
        ),
    ),
    second_stage_modules=[
        dict(type="BEVFeatureExtractor", pc_start=[-75.2, -75.2], voxel_size=[0.1, 0.1], out_stride=8)
    ],
    roi_head=dict(
        type="RoIHead",
        input_channels=128 * 5,
        model_cfg=dict(
            CLASS_AGNOSTIC=True, SHARED_FC=[64, 32], CLS_FC=[32, 16], REG_FC=[16, 32], DP_RATIO=0.3,
            TARGET_CONFIG=dict(ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE='roi_iou',
                               CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55),
            LOSS_CONFIG=dict(CLS_LOSS='BinaryCrossEntropy', REG_LOSS='L1',
                             LOSS_WEIGHTS={'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0,
                                           'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]}),
        ),
        code_size=9,
    ),
    NMS_POST_MAXSIZE=500,
    num_point=5,
    freeze=True,
)

assigner = dict(target_assigner=target_assigner, out_size_factor=get_downsample_factor(model), dense_reg=1,
                gaussian_overlap=0.1, max_objs=500, min_radius=2)
train_cfg = dict(assigner=assigner)
test_cfg = dict(
    post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0],
    max_per_img=4096,
    nms=dict(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=4096, nms_post_max_size=500,
             nms_iou_threshold=0.7),
    score_threshold=0.1,
    pc_range=[-75.2, -75.2],
    out_size_factor=get_downsample_factor(model),
    voxel_size=[0.1, 0.1],
)

dataset_type = "WaymoDataset"
nsweeps = 2
data_root = "DATA_ROOT"
val_preprocessor = dict(mode="PREPROCESS_MODE", shuffle_points=SHUFFLE_POINTS)
voxel_generator = dict(range=[-75.2, -75.2, -2, 75.2, 75.2, 4], voxel_size=[0.1, 0.1, 0.15], max_points_in_voxel=5,
                       max_voxel_num=[180000, 400000])
test_pipeline = [
    dict(type="LoadPointCloudFromFile", dataset=dataset_type),
    dict(type="LoadPointCloudAnnotations", with_bbox=True),
    dict(type="Preprocess", cfg=val_preprocessor),
    dict(type="Voxelization", cfg=voxel_generator),
    dict(type="AssignLabel", cfg=train_cfg["assigner"]),
    dict(type="Reformat"),
]
val_anno = "DATA_ROOT/infos_val_02sweeps_filter_zero_gt.pkl"
data = dict(
    samples_per_gpu=4,
    workers_per_gpu=4,
    val=dict(type=dataset_type, root_path=data_root, info_path=val_anno, test_mode=True, ann_file=val_anno, nsweeps=nsweeps,
             class_names=class_names, pipeline=test_pipeline),
)
device_ids = range(8)
log_level = "INFO"
work_dir = './work_dirs/{}/'.format(__file__[__file__.rfind('/') + 1:-3])
'''


def write_config(tmp_path, mode="val", shuffle=False, name="tiny_two_stage.py"):
    path = tmp_path / name
    path.write_text(TEXT.replace("DATA_ROOT", str(tmp_path)).replace("PREPROCESS_MODE", mode).replace("SHUFFLE_POINTS", str(shuffle)))
    return str(path)


def test_fromfile_access_and_what_it_leaves_behind(tmp_path):
    modules, path = dict(sys.modules), list(sys.path)
    cfg = config.Config.fromfile(write_config(tmp_path))
    assert sys.path == path and set(sys.modules) == set(modules)
    assert all(sys.modules[k] is v for k, v in modules.items()) and "det3d" not in sys.modules
    # attribute and item access, all the way down
    assert cfg.model.type == cfg["model"]["type"] == "TwoStageDetector"
    assert cfg.model.first_stage_cfg.neck.ds_layer_strides == [1, 2] and cfg.model["first_stage_cfg"].backbone["ds_factor"] == 8
    assert cfg.assigner.out_size_factor == 8 and cfg.test_cfg.out_size_factor == 8 and cfg.test_cfg["nms"].nms_iou_threshold == 0.7
    assert cfg.model.first_stage_cfg.bbox_head.common_heads.vel == (2, 2)
    assert cfg.test_pipeline[2].cfg.mode == "val" and cfg.data.val.pipeline[3]["cfg"].max_voxel_num == [180000, 400000]
    assert cfg.class_names == ["VEHICLE", "PEDESTRIAN", "CYCLIST"] and cfg.data.samples_per_gpu == 4
    assert cfg.work_dir == "./work_dirs/tiny_two_stage/" and cfg.filename.endswith("tiny_two_stage.py") and "nsweeps = 2" in cfg.text
    assert "model" in cfg and "nothing" not in cfg and len(cfg) > 10 and "tasks" in list(cfg)
    with pytest.raises(AttributeError, match="no attribute 'nothing'"):
        cfg.model.nothing
    with pytest.raises(KeyError):
        cfg.model["nothing"]
    cfg.local_rank = 0
    cfg.extra = dict(a=dict(b=1))
    assert cfg["local_rank"] == 0 and cfg.extra.a.b == 1
    # a module of the name that was there before is put back
    marker = type(sys)("det3d")
    sys.modules["det3d"] = marker
    try:
        config.Config.fromfile(write_config(tmp_path))
        assert sys.modules["det3d"] is marker and "det3d.utils" not in sys.modules
    finally:
        del sys.modules["det3d"]
    with pytest.raises(FileNotFoundError):
        config.Config.fromfile(str(tmp_path / "absent.py"))


def test_downsample_factor():
    f = config.get_downsample_factor
    one = dict(neck=dict(ds_layer_strides=[2, 2, 2], us_layer_strides=[1, 2, 4]), backbone=dict(ds_factor=1))
    assert f(one) == 2 and f(dict(first_stage_cfg=one)) == 2
    assert f(dict(neck=dict(), backbone=dict(ds_factor=8))) == 8


def test_the_data_set_reads_the_pipeline_and_refuses_training_preprocessing(tmp_path):
    cfg = config.Config.fromfile(write_config(tmp_path))
    infos = [{"path": f"p{i}", "anno_path": f"a{i}", "token": f"seq_0_frame_{i}.pkl", "timestamp": 0.1 * i,
              "sweeps": [{"path": f"p{max(i - 1, 0)}", "transform_matrix": None, "time_lag": 0}]} for i in range(5)]
    with open(cfg.data.val.info_path, "wb") as f:
        pickle.dump(infos, f)
    args = dict(cfg.data.val)
    assert args.pop("type") == "WaymoDataset"
    ds = waymo.WaymoDataset(**args)
    assert len(ds) == 5 and ds._num_point_features == 6 and ds.nsweeps == 2
    assert ds.voxel_generator["max_voxels"] == 400000 and ds.voxel_generator["max_points_in_voxel"] == 5
    assert ds.metadata(3) == {"image_prefix": str(tmp_path), "num_point_features": 6, "token": "seq_0_frame_3.pkl"}
    assert ds.sweeps(3) == [("p3", None, 0.0), ("p2", None, 0)]
    assert len(waymo.WaymoDataset(**dict(args, load_interval=2))) == 3
    assert waymo.WaymoDataset(**dict(args, nsweeps=1))._num_point_features == 5
    assert waymo.reorganize_info(infos)["seq_0_frame_2.pkl"] is infos[2]
    with pytest.raises(AssertionError, match="nsweeps 3 should be equal to the list length 1."):
        waymo.WaymoDataset(**dict(args, nsweeps=3)).sweeps(0)
    for kw, reason in ((dict(mode="train"), "mode='train'.*val pass-through"), (dict(shuffle=True), "shuffle_points=True.*file order")):
        bad = config.Config.fromfile(write_config(tmp_path, name="bad.py", **kw))
        with pytest.raises(ValueError, match=reason):
            waymo.WaymoDataset(**{k: v for k, v in bad.data.val.items() if k != "type"})
    with pytest.raises(ValueError, match="'GlobalRotation' is not read here"):
        waymo.WaymoDataset(**dict(args, pipeline=[dict(type="GlobalRotation")]))
    with pytest.raises(NotImplementedError, match="test_mode=False"):
        waymo.WaymoDataset(**dict(args, test_mode=False))


@pytest.fixture(scope="module")
def built(tmp_path_factory, request):
    tmp = tmp_path_factory.mktemp("cfg")
    cfg = config.Config.fromfile(write_config(tmp))
    return cfg, config.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg, voxel_generator=cfg.voxel_generator)


def test_a_missing_pretrained_prints_the_references_line_and_builds(tmp_path, capsys):
    cfg = config.Config.fromfile(write_config(tmp_path))
    model = config.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg, voxel_generator=cfg.voxel_generator)
    assert "no pretrained model at work_dirs/not_there/epoch_36.pth" in capsys.readouterr().out
    assert isinstance(model, two_stage.TwoStageDetector) and isinstance(model.single_det, detector.VoxelNet)
    det = model.single_det
    assert (det.max_points, det.max_voxels) == (5, 400000), "max_voxels is the val capacity, the second entry"
    assert det.voxel_size == [0.1, 0.1, 0.15] and det.pc_range == [-75.2, -75.2, -2, 75.2, 75.2, 4]
    assert model.roi_head.code_size == 9 and model.num_point == 5 and model.freeze and model.NMS_POST_MAXSIZE == 500
    assert det.test_cfg["nms"]["nms_iou_threshold"] == 0.7 and type(det.test_cfg) is dict
    # the classes' own door stays strict
    with pytest.raises(FileNotFoundError):
        detector.VoxelNet(**{k: v for k, v in cfg.model.first_stage_cfg.to_dict().items() if k != "type"})
    # a keyword no class knows is refused by name
    odd = cfg.model.to_dict()
    odd["first_stage_cfg"]["neck"]["dilation"] = 2
    config.build_detector(odd)                              # RPN takes the reference's **kwargs
    odd["roi_head"]["pooling"] = "max"
    with pytest.raises(TypeError, match="pooling"):
        config.build_detector(odd)
    with pytest.raises(KeyError, match="'SECOND' is not built here"):
        config.build_detector(dict(type="SECOND"))


def test_load_checkpoint(built, tmp_path, capsys):
    cfg, model = built
    sd = OrderedDict((k, torch.full_like(v, 3) if v.dtype.is_floating_point else v.clone()) for k, v in model.state_dict().items())
    key = "roi_head.cls_layers.7.bias"
    assert key in sd and "single_det.neck.blocks.0.1.weight" in sd

    def fresh():
        m = config.build_detector(cfg.model, test_cfg=cfg.test_cfg)
        capsys.readouterr()
        return m
    # {"state_dict": ...} with the module. prefix of a DataParallel run
    path = str(tmp_path / "dp.pth")
    torch.save({"state_dict": OrderedDict(("module." + k, v) for k, v in sd.items()), "meta": {"epoch": 6}}, path)
    m = fresh()
    ckpt = config.load_checkpoint(m, path)
    assert ckpt["meta"] == {"epoch": 6} and capsys.readouterr().out == ""
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    # the bare dict; a size mismatch, an unexpected and a missing key: reported, skipped, the rest loaded
    odd = OrderedDict(sd)
    odd[key] = torch.zeros(7)
    odd["roi_head.extra"] = torch.zeros(1)
    del odd["single_det.neck.blocks.0.1.weight"]
    del odd["single_det.neck.blocks.0.2.num_batches_tracked"]            # not missed
    path = str(tmp_path / "bare.pth")
    torch.save(odd, path)
    m = fresh()
    before = m.state_dict()[key].clone()
    config.load_checkpoint(m, path)
    out = capsys.readouterr().out
    assert "The model and loaded state dict do not match exactly" in out
    assert "unexpected key in source state_dict: roi_head.extra" in out
    assert "missing keys in source state_dict: single_det.neck.blocks.0.1.weight\n" in out
    assert "these keys have mismatched shape:" in out and key in out and "torch.Size([7])" in out
    assert torch.equal(m.state_dict()[key], before) and torch.equal(m.state_dict()["roi_head.cls_layers.7.weight"], sd["roi_head.cls_layers.7.weight"])
    with pytest.raises(RuntimeError, match="do not match exactly"):
        config.load_checkpoint(fresh(), path, strict=True)
    with pytest.raises(IOError, match="is not a checkpoint file"):
        config.load_checkpoint(m, str(tmp_path / "absent.pth"))
    torch.save({"weights": sd}, str(tmp_path / "none.pth"))
    with pytest.raises(RuntimeError, match="No state_dict found"):
        config.load_checkpoint(m, str(tmp_path / "none.pth"))


def test_dist_test_parser_and_refusals(tmp_path, monkeypatch):
    dist_test = importlib.import_module("3dal_pytorch_amd.dist_test")
    a = dist_test.parse_args(["cfg.py", "--work_dir", "w/val", "--checkpoint", "c.pth", "--speed_test", "--gpus", "1",
                              "--launcher", "none", "--local_rank", "0", "--txt_result", ""])
    assert (a.config, a.work_dir, a.checkpoint, a.speed_test, a.testset, a.mytrain) == ("cfg.py", "w/val", "c.pth", True, False, False)
    assert (a.precision, a.sparse_precision) == ("fp32", "fp32")
    assert dist_test.parse_args(["c.py", "--work_dir", "w", "--precision", "bf16", "--sparse_precision", "fp16"]).precision == "bf16"
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="single-process"):
        dist_test.main([write_config(tmp_path), "--work_dir", str(tmp_path / "val"), "--checkpoint", "c.pth"])
    assert os.environ["WORLD_SIZE"] == "2"
