"""`PointPillars` (3dal_pytorch_amd/detector.py) on the GPU: a seeded two-sample sweep on a 36 x 44 grid through
`forward(example)` and through `detect(points, offsets)`, against the same stages composed by hand — reader canvas -> RPN ->
CenterHead -> CenterHeadPost.predict — bit for bit, so that no score or IoU threshold makes the comparison conditional;
the reference-keyed checkpoint loads strictly; the metadata reaches `to_prediction`."""
import importlib

import numpy as np
import pytest
import torch

import pillars_ref as P
import rpn_ref as R
from _common import golden
from rpn_gpu import _dev, _record_file  # noqa: F401

pillars = importlib.import_module("3dal_pytorch_amd.pillars")
detector = importlib.import_module("3dal_pytorch_amd.detector")
detect = importlib.import_module("3dal_pytorch_amd.detect")
pytestmark = pytest.mark.gpu

VOXEL, RANGE = (0.32, 0.32, 6.0), (0.0, -5.76, -2.0, 14.08, 5.76, 4.0)      # 44 x 36 pillars
COUNTS = (3000, 1900)
TEST_CFG = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0],
                nms=dict(nms_pre_max_size=1000, nms_post_max_size=83, nms_iou_threshold=0.2), score_threshold=0.3,
                pc_range=[RANGE[0], RANGE[1]], out_size_factor=1, voxel_size=[0.32, 0.32])
MODEL = dict(reader=dict(type="PillarFeatureNet", num_filters=[64, 64], num_input_features=5, with_distance=False,
                         voxel_size=VOXEL, pc_range=RANGE),
             backbone=dict(type="PointPillarsScatter", ds_factor=1), neck=dict(type="RPN", **R.NECK),
             bbox_head=dict(type="CenterHead", **R.HEAD))
META = [{"token": "seq0_frame7", "num_point_features": 5}, {"token": "seq0_frame8", "num_point_features": 5}]


def checkpoint():
    sd = {"reader." + k: v for k, v in P.reader_weights(2, 5).items()}
    sd.update({"neck." + k: v for k, v in R.neck_weights().items()})
    sd.update({"bbox_head." + k: v for k, v in R.head_weights().items()})
    return {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}


def sweep():
    n = sum(COUNTS)
    lo, hi = np.asarray(RANGE[:3]), np.asarray(RANGE[3:])
    xyz = P.synth.uniform(R.SEED, "sweep/xyz", (n, 3)) * (hi - lo) * 1.04 + lo - 0.02 * (hi - lo)       # a few fall outside
    pts = np.concatenate([xyz, P.synth.uniform(R.SEED, "sweep/f", (n, 2))], 1).astype(np.float32)
    return pts, np.asarray([0, COUNTS[0], n], np.int64)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    path = tmp_path_factory.mktemp("ckpt") / "latest.pth"
    torch.save({"state_dict": checkpoint(), "meta": {"epoch": 36}}, path)
    m = detector.PointPillars(**MODEL, test_cfg=TEST_CFG, pretrained=str(path), max_points=20, max_voxels=2000)
    return m.cuda().eval()


def _same(a, b):
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        assert set(x) == set(y) == {"box3d_lidar", "scores", "label_preds", "metadata"}
        for k in ("box3d_lidar", "scores", "label_preds"):
            assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), k
        assert x["metadata"] is y["metadata"]


def test_checkpoint_keys_are_the_references_and_load_strictly(model):
    g = golden("rpn")
    sd = checkpoint()
    assert set(sd) == {str(k) for k in g["keys"]} == set(model.state_dict())
    fresh = detector.PointPillars(**MODEL)
    fresh.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError, match="Missing key"):
        fresh.load_state_dict({k: v for k, v in sd.items() if k != "neck.deblocks.2.1.running_var"}, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k


def test_forward_and_detect_equal_the_stages_composed_by_hand(model):
    pts, off = sweep()
    dpts = _dev(pts)
    # ---- by hand
    r = pillars.voxelize(dpts, off, VOXEL, RANGE, 20, 2000)
    canvas = model.reader.forward_canvas(r.voxels, r.num_points, r.coordinates, 2, [44, 36], n_pillars=r.n_pillars)
    assert canvas.shape == (2, 64, 36, 44)
    torch.cuda.synchronize()
    model.neck.packed(), model.bbox_head.packed()
    torch.cuda.set_sync_debug_mode("error")     # the dense stage is enqueued without a host synchronisation
    try:
        with torch.no_grad():
            preds = model.bbox_head(model.neck(canvas))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not preds[0]["hm"].is_contiguous()   # a channel slice of the task's one tensor: decode reads it through strides
    want = detect.CenterHeadPost(TEST_CFG, [3]).predict(preds, metadata=META)
    n = [int(w["scores"].numel()) for w in want]
    assert all(0 < k <= 83 for k in n) and max(n) > 10, n
    assert want[0]["box3d_lidar"].shape[1] == 7 and set(torch.cat([w["label_preds"] for w in want]).tolist()) == {0, 1, 2}
    # ---- forward(example): the reference's collated batch
    voxels, coords, num, nv = r.finish()
    example = dict(voxels=voxels, coordinates=coords, num_points=num, num_voxels=nv, shape=[[44, 36, 1]] * 2, metadata=META)
    with torch.no_grad():
        _same(model(example, return_loss=False), want)
        _same(model(example), want)
    # ---- detect(points, offsets)
    got = model.detect(dpts, off, metadata=META)
    _same(got, want)
    assert int(model.last.voxel_offsets[-1]) == voxels.shape[0]
    pred = model.to_prediction(got)
    assert list(pred) == ["seq0_frame7", "seq0_frame8"]
    for i, (token, out) in enumerate(pred.items()):
        assert out["metadata"] is META[i] and not out["box3d_lidar"].is_cuda
        assert torch.equal(out["box3d_lidar"], want[i]["box3d_lidar"].cpu()) and torch.equal(out["scores"], want[i]["scores"].cpu())
    none = model.detect(dpts, off)
    assert none[0]["metadata"] is None and torch.equal(none[1]["scores"], want[1]["scores"])
    with pytest.raises(NotImplementedError, match="loss is not built"):
        model(example, return_loss=True)
    with pytest.raises(RuntimeError, match="eval-mode"):
        model.train().detect(dpts, off)
    model.eval()
