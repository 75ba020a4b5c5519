"""`TwoStageDetector` (3dal_pytorch_amd/two_stage.py) end to end on the GPU, on tests/test_gpu_voxelnet.py's grid, sweep and
seeded checkpoint scheme extended with seeded roi_head.* values: `detect(points, offsets)`, `forward(example)` and the
stages one by one — the first stage's modules, CenterHeadPost.predict, get_box_center, BEVFeatureExtractor,
reorder_first_stage_pred_and_feature, RoIHead, post_process — bit for bit, so that no threshold makes the comparison
conditional. The checkpoint round trip goes through `init_weights` with the duplicated bbox_head.* keys present. One case
runs with a PointPillars first stage (tests/test_gpu_detector.py's)."""
import importlib

import numpy as np
import pytest
import torch

import roi_ref as R
import test_gpu_detector as PP
import test_gpu_voxelnet as V
from roi_gpu import _dev, _record_file  # noqa: F401

pillars = importlib.import_module("3dal_pytorch_amd.pillars")
detect = importlib.import_module("3dal_pytorch_amd.detect")
two_stage = importlib.import_module("3dal_pytorch_amd.two_stage")
pytestmark = pytest.mark.gpu

M = 83                                          # nms_post_max_size of the one task: a sample cannot overflow
ROI_CFG = R.model_cfg([64, 32], [32, 16], [16, 32])


def two_stage_cfg(first, channels, num_point, voxel, pc_start, out_stride):
    return dict(first_stage_cfg=first,
                second_stage_modules=[dict(type="BEVFeatureExtractor", pc_start=list(pc_start), voxel_size=list(voxel), out_stride=out_stride)],
                roi_head=dict(type="RoIHead", input_channels=channels * num_point, model_cfg=ROI_CFG, code_size=7),
                NMS_POST_MAXSIZE=M, num_point=num_point, freeze=True)


def checkpoint(first_sd, channels, tag):
    """a reference-style two-stage checkpoint: single_det.*, the duplicated bbox_head.*, and seeded roi_head.*"""
    sd = {"single_det." + k: v for k, v in first_sd.items()}
    sd.update({k: v for k, v in first_sd.items() if k.startswith("bbox_head.")})
    sd.update({"roi_head." + k: torch.as_tensor(np.asarray(v)) for k, v in R.head_weights(channels, ROI_CFG, 7, tag).items()})
    return sd


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    path = tmp_path_factory.mktemp("ckpt2") / "latest.pth"
    sd = checkpoint(V.checkpoint(), 128 * 5, "e2e")
    torch.save({"state_dict": sd, "meta": {"epoch": 6}}, path)
    cfg = two_stage_cfg(dict(type="VoxelNet", **V.MODEL), 128, 5, V.VOXEL[:2], V.RANGE[:2], 8)
    m = two_stage.TwoStageDetector(**cfg, test_cfg=V.TEST_CFG, pretrained=str(path), **V.KW)
    return m.cuda().eval(), sd


def _stages(m, preds, bev, meta):
    """the reference's forward after the head, module by module"""
    first = detect.CenterHeadPost(m.test_cfg, m.bbox_head.num_classes).predict(preds, metadata=meta)
    centres = m.get_box_center(first)
    feats = m.second_stage[0]({"bev_feature": bev.permute(0, 2, 3, 1)}, centres, m.num_point)
    example = m.reorder_first_stage_pred_and_feature(first, {"metadata": meta}, [feats])
    return first, m.post_process(m.roi_head(example, training=False))


def test_checkpoint_round_trip_with_the_duplicated_head_keys(model):
    m, sd = model
    assert set(sd) == set(m.state_dict())
    assert {k.split(".")[0] for k in sd} == {"single_det", "bbox_head", "roi_head"}
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    assert m.bbox_head is m.single_det.bbox_head
    fresh = two_stage.TwoStageDetector(**two_stage_cfg(dict(type="VoxelNet", **V.MODEL), 128, 5, V.VOXEL[:2], V.RANGE[:2], 8))
    with pytest.raises(RuntimeError, match="Missing key"):
        fresh.load_state_dict({k: v for k, v in sd.items() if k != "roi_head.cls_layers.7.bias"}, strict=True)


def test_detect_equals_forward_equals_the_stages_one_by_one(model):
    m, _ = model
    det = m.single_det
    pts, off = V.sweep()
    dpts = _dev(pts)
    r = pillars.voxelize(dpts, off, V.VOXEL, V.RANGE, 5, 4000)
    voxels, coords, num, nv = r.finish()
    example = dict(voxels=voxels, coordinates=coords, num_points=num, num_voxels=nv, shape=[V.GRID] * 2, metadata=V.META)
    with torch.no_grad():
        bev, _ = det.extract_feat(dict(features=voxels, num_voxels=num, coors=coords, batch_size=2, input_shape=V.GRID))
        preds = m.bbox_head(bev)
        first, want = _stages(m, preds, bev, V.META)
    assert sum(int(w["scores"].numel()) for w in want) > 0 and bev.shape[1] == 128
    # counts and labels are the first stage's; the boxes are not
    for f, w in zip(first, want):
        assert w["scores"].numel() == f["scores"].numel() and torch.equal(w["label_preds"], f["label_preds"])
        assert w["label_preds"].dtype == torch.int64 and w["box3d_lidar"].shape == f["box3d_lidar"].shape
        assert w["scores"].numel() == 0 or not torch.equal(w["box3d_lidar"], f["box3d_lidar"])
    got = m(example, return_loss=False)                                       # warm
    V._same(got, want)
    # the second stage's device part may not synchronise (decode_nms uploads its segment offsets, which the debug mode
    # counts as one: it stays outside)
    r = m.post().decode_nms(preds)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = m.refine(r, bev)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(out["status"].item()) == 0 and out["counts"].tolist() == [int(w["scores"].numel()) for w in want]
    V._same(m.detect(dpts, off, metadata=V.META), want)
    assert list(m.to_prediction(got)) == ["seq0_frame7", "seq0_frame8"]
    with pytest.raises(NotImplementedError, match="loss is not built"):
        m(example, return_loss=True)
    with pytest.raises(RuntimeError, match="eval-mode"):
        m.train().detect(dpts, off)
    m.eval()


def test_point_pillars_first_stage(tmp_path):
    path = tmp_path / "pp.pth"
    torch.save({"state_dict": checkpoint(PP.checkpoint(), 384, "pp")}, path)
    cfg = two_stage_cfg(dict(type="PointPillars", **PP.MODEL), 384, 1, PP.VOXEL[:2], PP.RANGE[:2], 1)
    m = two_stage.TwoStageDetector(**cfg, test_cfg=PP.TEST_CFG, pretrained=str(path), max_points=20, max_voxels=2000).cuda().eval()
    pts, off = PP.sweep()
    dpts = _dev(pts)
    got = m.detect(dpts, off, metadata=PP.META)
    r = pillars.voxelize(dpts, off, PP.VOXEL, PP.RANGE, 20, 2000)
    voxels, coords, num, nv = r.finish()
    grid = pillars.grid_size(PP.VOXEL, PP.RANGE)
    with torch.no_grad():
        bev = m.single_det.extract_feat(dict(features=voxels, num_voxels=num, coors=coords, batch_size=2, input_shape=[int(g) for g in grid]))
        first, want = _stages(m, m.bbox_head(bev), bev, PP.META)
    assert sum(int(w["scores"].numel()) for w in want) > 0
    V._same(got, want)
    example = dict(voxels=voxels, coordinates=coords, num_points=num, num_voxels=nv, shape=[[int(g) for g in grid]] * 2, metadata=PP.META)
    V._same(m(example), want)
    assert all(torch.equal(w["label_preds"], f["label_preds"]) for f, w in zip(first, want))
    # fewer slots than a sample's kept boxes: the overflow bit, raised by name at the read-back
    assert max(int(w["scores"].numel()) for w in want) > 2
    small = two_stage.TwoStageDetector(m.single_det, [m.second_stage[0]], m.roi_head, 2, num_point=1, test_cfg=PP.TEST_CFG).eval()
    with pytest.raises(RuntimeError, match="NMS_POST_MAXSIZE = 2"):
        small.detect(dpts, off, metadata=PP.META)
