"""The detection run at file level (3dal_pytorch_amd/dist_test.py) on the GPU: a synthetic Waymo-style directory of two
sequences x three frames (synth.waymo_files), a config file in the reference's format and a seeded checkpoint, all written
under tmp_path, through `dist_test.main([...])`. The model is tests/test_gpu_voxelnet.py's grid, dicts and checkpoint under
tests/test_gpu_two_stage.py's two-stage wrapper, with num_input_features = 6 in the reader and the backbone (two sweeps: the
time column); one case is tests/test_gpu_detector.py's PointPillars with one sweep. prediction.pkl must hold, bit for bit,
what `model.detect` gives on the loader's own batches."""
import copy
import importlib
import pickle
import pprint

import numpy as np
import pytest
import torch

import sparse_ref as S
import test_gpu_detector as PP
import test_gpu_two_stage as TS
import test_gpu_voxelnet as V

config = importlib.import_module("3dal_pytorch_amd.config")
dist_test = importlib.import_module("3dal_pytorch_amd.dist_test")
synth = importlib.import_module("3dal_pytorch_amd.synth")
track = importlib.import_module("3dal_pytorch_amd.track")
waymo = importlib.import_module("3dal_pytorch_amd.waymo")
pytestmark = pytest.mark.gpu

KEYS = {"box3d_lidar", "scores", "label_preds", "metadata"}


def _floats(v):
    return [float(x) for x in v]


def write_config(path, model, test_cfg, voxel_generator, nsweeps, root, info_path):
    """a config in the reference's format: the model dict, the factor through get_downsample_factor, the val pipeline"""
    path.write_text(f'''import itertools
import logging

from det3d.utils.config_tool import get_downsample_factor

tasks = {V.TASKS!r}
class_names = list(itertools.chain(*[t["class_names"] for t in tasks]))
model = {pprint.pformat(model, width=120)}
assigner = dict(target_assigner=dict(tasks=tasks), out_size_factor=get_downsample_factor(model), dense_reg=1,
                gaussian_overlap=0.1, max_objs=500, min_radius=2)
train_cfg = dict(assigner=assigner)
test_cfg = dict({pprint.pformat(test_cfg, width=120)}, out_size_factor=get_downsample_factor(model))
dataset_type = "WaymoDataset"
nsweeps = {nsweeps}
data_root = {str(root)!r}
val_preprocessor = dict(mode="val", shuffle_points=False)
voxel_generator = {voxel_generator!r}
test_pipeline = [
    dict(type="LoadPointCloudFromFile", dataset=dataset_type),
    dict(type="LoadPointCloudAnnotations", with_bbox=True),
    dict(type="Preprocess", cfg=val_preprocessor),
    dict(type="Voxelization", cfg=voxel_generator),
    dict(type="AssignLabel", cfg=train_cfg["assigner"]),
    dict(type="Reformat"),
]
val_anno = {str(info_path)!r}
data = dict(
    samples_per_gpu=4,
    workers_per_gpu=4,
    val=dict(type=dataset_type, root_path=data_root, info_path=val_anno, test_mode=True, ann_file=val_anno, nsweeps=nsweeps,
             class_names=class_names, pipeline=test_pipeline),
    mytrain=dict(type=dataset_type, root_path=data_root, info_path=val_anno, test_mode=True, ann_file=val_anno,
                 nsweeps=nsweeps, class_names=class_names, pipeline=test_pipeline),
)
log_level = "INFO"
''')
    return str(path)


@pytest.fixture(scope="module")
def two_stage_run(tmp_path_factory):
    """the directory, the config, the checkpoint, and one run into .../val"""
    root = tmp_path_factory.mktemp("dist_test")
    # seed and size: the seeded weights regress most centres out of post_center_limit_range, the more so the denser the
    # grid is filled; on this draw three of the six frames keep boxes (3, 0, 0, 4, 0, 1), which _check_prediction asserts
    info_path, infos = synth.waymo_files(str(root / "data"), 3, n_sequences=2, n_frames=3, n_points=1500, nsweeps=2, pc_range=V.RANGE)
    first = copy.deepcopy(V.MODEL)
    first["reader"]["num_input_features"] = first["backbone"]["num_input_features"] = 6
    first["neck"]["logger"] = "LOGGER"
    model = TS.two_stage_cfg(dict(type="VoxelNet", **first), 128, 5, V.VOXEL[:2], V.RANGE[:2], 8)
    model = dict(type="TwoStageDetector", **model)
    text_model = copy.deepcopy(model)
    cfg_path = root / "tiny_two_sweep_two_stage.py"
    generator = dict(range=_floats(V.RANGE), voxel_size=_floats(V.VOXEL), max_points_in_voxel=5, max_voxel_num=[3000, 4000])
    test_cfg = {k: v for k, v in V.TEST_CFG.items() if k != "out_size_factor"}
    write_config(cfg_path, text_model, test_cfg, generator, 2, root / "data", info_path)
    # the configs pass a logger to the neck: written as the call it is
    cfg_path.write_text(cfg_path.read_text().replace("'LOGGER'", 'logging.getLogger("RPN")'))
    first_sd = V.checkpoint()
    first_sd.update({"backbone." + k: torch.as_tensor(np.asarray(v)) for k, v in S.backbone_weights(6).items()})
    ckpt = root / "CenterPoint.pth"
    torch.save({"state_dict": {"module." + k: v for k, v in TS.checkpoint(first_sd, 128 * 5, "e2e").items()}, "meta": {"epoch": 6}}, ckpt)
    work = root / "work" / "val"
    got = dist_test.main([str(cfg_path), "--work_dir", str(work), "--checkpoint", str(ckpt)])
    return dict(root=root, cfg=str(cfg_path), ckpt=str(ckpt), work=work, infos=infos, returned=got)


def _direct(cfg_path, ckpt, batch_size, precision="fp32", sparse_precision="fp32"):
    """model.detect on the loader's own batches, built as the run builds them"""
    cfg = config.Config.fromfile(cfg_path)
    dataset = dist_test.build_dataset(cfg.data.val)
    model = config.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg, voxel_generator=dataset.voxel_generator)
    config.load_checkpoint(model, ckpt, map_location="cpu")
    model = model.cuda().eval()
    model.precision = precision
    if sparse_precision != "fp32":                          # a detector without a sparse middle refuses the knob
        model.sparse_precision = sparse_precision
    out = []
    for points, offsets, offsets_device, metadata in waymo.SweepLoader(dataset, batch_size, "cuda"):
        assert points.shape[1] == dataset._num_point_features
        out += model.detect(points, offsets, metadata, offsets_device)
    return cfg, out


class Spy:
    """what a run of dist_test.main built: every SweepLoader's batch size and the samples of each batch it yielded, and
    every model build_detector returned"""

    def __init__(self, monkeypatch):
        self.batch_sizes, self.batches, self.models = [], [], []
        spy, loader, build = self, waymo.SweepLoader, config.build_detector

        class Loader(loader):
            def __init__(self, dataset, batch_size, device, capacity=None):
                spy.batch_sizes.append(batch_size)
                super().__init__(dataset, batch_size, device, capacity)

            def __iter__(self):
                for batch in super().__iter__():
                    spy.batches.append(len(batch[3]))
                    yield batch

        def build_detector(*args, **kwargs):
            spy.models.append(build(*args, **kwargs))
            return spy.models[-1]
        monkeypatch.setattr(waymo, "SweepLoader", Loader)
        monkeypatch.setattr(config, "build_detector", build_detector)


def _check_prediction(pred, infos, cols):
    assert list(pred) == [i["token"] for i in infos], "every token, in data-set order"
    for tok, p in pred.items():
        assert set(p) == KEYS and p["metadata"]["token"] == tok
        assert all(torch.is_tensor(p[k]) and p[k].device.type == "cpu" for k in KEYS - {"metadata"})
        assert p["label_preds"].dtype == torch.int64 and p["box3d_lidar"].dtype == p["scores"].dtype == torch.float32
        assert p["box3d_lidar"].shape == (p["scores"].numel(), cols) and p["label_preds"].shape == p["scores"].shape
    kept = [int(p["scores"].numel()) for p in pred.values()]
    print("kept boxes per frame:", kept)
    assert max(kept) > 0, "no frame keeps a box: the comparison would be empty"


def _check_det_annos(det_annos, pred, infos, n):
    assert len(det_annos) == n
    for a, info in zip(det_annos, infos[:n]):
        p = pred[info["token"]]
        box = p["box3d_lidar"].numpy()
        assert a["boxes_lidar"].shape == (box.shape[0], 7)
        assert np.array_equal(a["boxes_lidar"][:, [3, 4]], box[:, [4, 3]]), "l and w swapped back to Waymo's order"
        assert np.array_equal(a["boxes_lidar"][:, 6], -box[:, -1] - np.pi / 2) and np.array_equal(a["boxes_lidar"][:, :3], box[:, :3])
        assert np.array_equal(a["score"], p["scores"].numpy())
        assert list(a["name"]) == [track.LABEL_TO_NAME[int(i)] for i in p["label_preds"]]
        with open(info["anno_path"], "rb") as f:
            obj = pickle.load(f)
        assert a["frame_id"] == f"segment-{obj['scene_name']}_with_camera_labels_{obj['frame_id']:03d}"
        assert a["metadata"] == {"context_name": obj["scene_name"], "timestamp_micros": int(str(info["timestamp"]).replace(".", ""))}


def test_prediction_pkl_is_detect_on_the_loaders_batches(two_stage_run):
    r = two_stage_run
    with open(r["work"] / "prediction.pkl", "rb") as f:
        pred = pickle.load(f)
    _check_prediction(pred, r["infos"], 7)
    cfg, want = _direct(r["cfg"], r["ckpt"], 4)
    assert cfg.data.samples_per_gpu == 4 and cfg.test_cfg.out_size_factor == V.TEST_CFG["out_size_factor"]
    assert len(want) == len(pred) == 6
    for w in want:
        p = pred[w["metadata"]["token"]]
        for k in ("box3d_lidar", "scores", "label_preds"):
            assert p[k].dtype == w[k].dtype and torch.equal(p[k], w[k].cpu()), (w["metadata"]["token"], k)
        assert p["metadata"] == w["metadata"]
    assert set(r["returned"]) == set(pred)
    # det_annos.pkl, and the tracking run's door to prediction.pkl
    with open(r["work"] / "det_annos.pkl", "rb") as f:
        _check_det_annos(pickle.load(f), pred, r["infos"], 6)
    assert not (r["work"] / "detection_pred.bin").exists()
    loaded = track._load(str(r["work"] / "prediction.pkl"))
    tok = r["infos"][0]["token"]
    assert track._np(loaded[tok]["box3d_lidar"]).dtype == np.float32 and track._np(loaded[tok]["label_preds"]).dtype == np.int64
    assert track.sort_order(list(loaded)) == list(range(6))


def test_the_batch_size_is_the_configs_and_the_precision_knobs_reach_the_model(two_stage_run, monkeypatch):
    r = two_stage_run
    spy = Spy(monkeypatch)
    work = r["root"] / "work16" / "val"
    pred = dist_test.main([r["cfg"], "--work_dir", str(work), "--checkpoint", r["ckpt"], "--precision", "bf16",
                           "--sparse_precision", "fp16"])
    assert spy.batch_sizes == [4] and spy.batches == [4, 2], "samples_per_gpu = 4 over six frames"
    model, = spy.models
    assert (model.precision, model.sparse_precision) == ("bf16", "fp16") and not model.training
    assert (model.single_det.neck.precision, model.single_det.bbox_head.precision) == ("bf16", "bf16")
    assert model.single_det.backbone.sparse_precision == "fp16"
    monkeypatch.undo()
    _check_prediction(pred, r["infos"], 7)
    _, want = _direct(r["cfg"], r["ckpt"], 4, "bf16", "fp16")
    for w in want:
        for k in ("box3d_lidar", "scores", "label_preds"):
            assert torch.equal(pred[w["metadata"]["token"]][k], w[k].cpu()), k
    # the 16-bit operands are really in use: some score differs from the fp32 run's
    fp32 = r["returned"]
    assert any(p["scores"].shape != fp32[t]["scores"].shape or not torch.equal(p["scores"], fp32[t]["scores"]) for t, p in pred.items())


def test_a_train_work_dir_keeps_the_first_quarter_and_speed_test_runs_frame_by_frame(two_stage_run, capsys, monkeypatch):
    r = two_stage_run
    spy = Spy(monkeypatch)
    work = r["root"] / "work" / "train"
    pred = dist_test.main([r["cfg"], "--work_dir", str(work), "--checkpoint", r["ckpt"], "--speed_test", "--mytrain"])
    assert spy.batch_sizes == [1] and spy.batches == [1] * 6, "--speed_test: one frame a batch whatever samples_per_gpu says"
    assert (spy.models[0].precision, spy.models[0].sparse_precision) == ("fp32", "fp32")
    monkeypatch.undo()
    out = capsys.readouterr().out
    assert "Use Train Set" in out and "Total time per frame:" in out and "detection_pred.bin is skipped" in out
    assert out.index("Saved prediction.pkl") < out.index("Saved det_annos.pkl")
    _check_prediction(pred, r["infos"], 7)
    with open(work / "det_annos.pkl", "rb") as f:
        _check_det_annos(pickle.load(f), pred, r["infos"], int(6 * 0.25))
    with open(work / "prediction.pkl", "rb") as f:
        assert list(pickle.load(f)) == list(pred)
    # batch size 1: the same frames one by one
    _, want = _direct(r["cfg"], r["ckpt"], 1)
    for w in want:
        for k in ("box3d_lidar", "scores", "label_preds"):
            assert torch.equal(pred[w["metadata"]["token"]][k], w[k].cpu()), k


def test_point_pillars_one_sweep(tmp_path, capsys):
    info_path, infos = synth.waymo_files(str(tmp_path / "data"), 12, n_sequences=1, n_frames=3, n_points=3000, nsweeps=1, pc_range=PP.RANGE)
    model = dict(type="PointPillars", **copy.deepcopy(PP.MODEL))
    generator = dict(range=_floats(PP.RANGE), voxel_size=_floats(PP.VOXEL), max_points_in_voxel=20, max_voxel_num=[1500, 2000])
    test_cfg = {k: v for k, v in PP.TEST_CFG.items() if k != "out_size_factor"}
    cfg_path = write_config(tmp_path / "tiny_pp.py", model, test_cfg, generator, 1, tmp_path / "data", info_path)
    ckpt = tmp_path / "pp.pth"
    torch.save({"state_dict": PP.checkpoint()}, ckpt)
    work = tmp_path / "work" / "val"
    pred = dist_test.main([cfg_path, "--work_dir", str(work), "--checkpoint", str(ckpt)])
    assert "Use Val Set" in capsys.readouterr().out
    _check_prediction(pred, infos, 7)
    cfg, want = _direct(cfg_path, str(ckpt), 4)
    assert cfg.test_cfg.out_size_factor == PP.TEST_CFG["out_size_factor"] and len(want) == 3
    for w in want:
        for k in ("box3d_lidar", "scores", "label_preds"):
            assert torch.equal(pred[w["metadata"]["token"]][k], w[k].cpu()), k
    with open(work / "det_annos.pkl", "rb") as f:
        _check_det_annos(pickle.load(f), pred, infos, 3)
