"""dal3_nms on the GPU (3dal_pytorch_amd/nms.py): the kept rows the reference's own rotate_nms_pcdet / circle_nms
recorded (tests/golden/nms.npz), the bit-exact contract against the package's own IoU entry (a host greedy scan over
iou.boxes_iou_bev of the sorted boxes, downloaded), planted cases, and the independence of the result from the batching,
the grid and the run."""
import importlib

import numpy as np
import pytest
import torch

import nms_ref
from _common import golden

hip = importlib.import_module("3dal_pytorch_amd._hip")
iou = importlib.import_module("3dal_pytorch_amd.iou")
nms = importlib.import_module("3dal_pytorch_amd.nms")
pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scene(n, seed, dtype=np.float32):
    """n clustered boxes with distinct scores; float64 boxes carry digits float32 cannot hold"""
    boxes, scores = nms_ref.clustered_scene(seed, n_objects=max(1, n))
    assert boxes.shape[0] >= n
    boxes, scores = boxes[:n], scores[:n]
    if dtype == np.float64:
        boxes = boxes.astype(np.float64) + np.random.default_rng(seed).normal(0, 1e-6, boxes.shape)
    return boxes, scores


def host_greedy(boxes, scores, thresh, pre_max=0, post_max=0, mirror=False):
    """the contract: greedy scan over the package's own pairwise IoU of the sorted candidates, > thresh in float32"""
    o = nms_ref.order(scores)
    if pre_max:
        o = o[:pre_max]
    b = boxes[o]
    if mirror:
        b = nms_ref.mirrored(b)
    m = iou.boxes_iou_bev(dev(b), dev(b)).cpu().numpy() if o.size else np.zeros((0, 0), np.float32)
    with np.errstate(invalid="ignore"):
        return o[nms_ref.greedy(m > np.float32(thresh), post_max)]


def run_one(boxes, scores, mode, thresh, pre_max=0, post_max=0, **kw):
    keep, count = nms.batched_nms(dev(boxes), dev(scores), [0, boxes.shape[0]], mode, thresh, pre_max, post_max, **kw)
    assert keep.dtype == torch.int32 and count.dtype == torch.int32 and keep.is_cuda and count.is_cuda
    return keep[0, :int(count[0])].cpu().numpy().astype(np.int64)


# ---------------------------------------------------------------------------------- the reference's results
@pytest.mark.parametrize("case", sorted(nms_ref.SCENE_CASES))
def test_kept_rows_equal_the_references(case):
    g = golden("nms")
    boxes, scores = nms_ref.clustered_scene(int(g["scene_seed"]))
    mode, thresh, pre, post = nms_ref.SCENE_CASES[case]
    want = g[f"scene_{case}_keep"]
    if mode == "rotate":
        got = nms.rotate_nms_pcdet(dev(boxes), dev(scores), thresh, pre_maxsize=pre, post_max_size=post)
        assert np.array_equal(run_one(boxes, scores, mode, thresh, pre, post, mirror=True), want)
    else:
        got = nms.circle_nms(dev(np.concatenate([boxes[:, :2], scores[:, None]], 1)), thresh, post_max_size=post)
        assert np.array_equal(run_one(boxes, scores, mode, thresh, pre, post), want)
    assert got.dtype == torch.int64 and got.is_cuda and got.dim() == 1
    assert np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------- bit-exact self-consistency
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 128, 129, 300, 255, 256, 257, 513])
def test_keep_is_the_greedy_scan_over_the_packages_own_iou(n, dtype):
    boxes, scores = scene(n, 100 + n, dtype)
    for thresh in (0.7, 0.2):
        assert np.array_equal(run_one(boxes, scores, "rotate", thresh), host_greedy(boxes, scores, thresh)), thresh
    assert np.array_equal(run_one(boxes, scores, "rotate", 0.5, mirror=True), host_greedy(boxes, scores, 0.5, mirror=True))


def test_three_distinct_scores_over_three_sort_tiles_go_by_row():
    """513 rows = two full 256-entry tiles of the one-workgroup sort and one entry: with three score values the order
    inside a score is the rows', across the waves of a tile and across the tiles"""
    boxes, _ = scene(513, 613)
    scores = np.array([0.25, 0.5, 0.75], np.float32)[np.random.default_rng(613).integers(0, 3, 513)]
    keep, count, order = nms.batched_nms(dev(boxes), dev(scores), [0, 513], "rotate", 0.7, return_order=True)
    assert np.array_equal(order.cpu().numpy(), nms_ref.order(scores))
    assert np.array_equal(keep[0, :int(count[0])].cpu().numpy(), host_greedy(boxes, scores, 0.7))


def test_large_segment_with_both_cuts():
    boxes, scores = scene(5000, 7)
    got = run_one(boxes, scores, "rotate", 0.7, 4096, 500)
    want = host_greedy(boxes, scores, 0.7, 4096, 500)
    assert want.size == 500 and np.array_equal(got, want)


def test_circle_is_the_float32_scan():
    for n in (1, 64, 65, 300):
        boxes, scores = scene(n, 300 + n)
        for thresh, post in ((1.0, 0), (0.25, 17)):
            assert np.array_equal(run_one(boxes, scores, "circle", thresh, 0, post),
                                  nms_ref.nms(boxes, scores, "circle", thresh, 0, post)), (n, thresh)


# ---------------------------------------------------------------------------------- planted cases
def row(x, y=0.0, yaw=0.0):
    return [x, y, 0.0, 4.0, 2.0, 1.5, yaw]


def test_chain_the_suppressed_box_suppresses_nobody():
    """IoU(A, B) = IoU(B, C) = 0.6, IoU(A, C) = 1/3 at 0.5: B goes, so C stays"""
    boxes = np.array([row(0.0), row(1.0), row(2.0)], np.float32)
    assert run_one(boxes, np.array([0.9, 0.8, 0.7], np.float32), "rotate", 0.5).tolist() == [0, 2]
    assert run_one(boxes, np.array([0.7, 0.9, 0.8], np.float32), "rotate", 0.5).tolist() == [1]


def test_tied_scores_go_by_row_and_nan_scores_first():
    far = np.array([row(20.0 * k) for k in range(6)], np.float32)
    s = np.array([0.5, 0.9, 0.5, np.nan, 0.5, -0.0], np.float32)
    keep, count, order = nms.batched_nms(dev(far), dev(s), [0, 6], "rotate", 0.7, return_order=True)
    assert order.cpu().tolist() == [3, 1, 0, 2, 4, 5] == nms_ref.order(s).tolist()
    assert keep[0, :int(count[0])].cpu().tolist() == [3, 1, 0, 2, 4, 5]
    s0 = np.array([0.0, -0.0, 0.0, -0.0], np.float32)                 # -0 == +0: a tie
    assert run_one(far[:4], s0, "rotate", 0.7).tolist() == [0, 1, 2, 3]
    same = np.array([row(0.0)] * 3, np.float32)                     # equal scores, identical boxes: the lowest row wins
    assert run_one(same, np.array([0.4, 0.4, 0.4], np.float32), "rotate", 0.7).tolist() == [0]
    assert run_one(same, np.array([0.4, np.nan, 0.9], np.float32), "rotate", 0.7).tolist() == [1]


def test_a_non_finite_box_is_kept_and_suppresses_nothing():
    boxes = np.array([row(0.0), row(np.nan), row(0.1), row(0.0, yaw=np.inf), row(0.2)], np.float32)
    s = np.array([0.5, 0.9, 0.8, 0.3, 0.2], np.float32)
    assert run_one(boxes, s, "rotate", 0.5).tolist() == [1, 2, 3]
    assert run_one(boxes.astype(np.float64), s, "rotate", 0.5).tolist() == [1, 2, 3]
    assert run_one(boxes, s, "circle", 1.0).tolist() == [1, 2]      # the yaw plays no part in a circle; a NaN x does


def test_identical_boxes_keep_the_best_only():
    boxes = np.array([row(3.0, 1.0, 0.3)] * 70, np.float32)         # more than one block of 64
    s = np.linspace(0.1, 0.9, 70).astype(np.float32)
    assert run_one(boxes, s, "rotate", 0.7).tolist() == [69]


def test_post_max_is_the_uncut_result_truncated():
    boxes, scores = scene(300, 11)
    full = run_one(boxes, scores, "rotate", 0.7)
    assert full.size > 66
    for post in (1, 7, 64, 65, full.size, full.size + 5):
        assert np.array_equal(run_one(boxes, scores, "rotate", 0.7, 0, post), full[:post]), post
    cut = run_one(boxes, scores, "rotate", 0.7, 100, 0)            # pre_max: a scan of the best 100 only
    assert np.array_equal(cut, host_greedy(boxes, scores, 0.7, 100)) and set(cut) <= set(nms_ref.order(scores)[:100])


def test_the_circle_compares_the_squared_distance_inclusively():
    boxes = np.array([row(0.0), row(1.0)], np.float32)
    s = np.array([0.9, 0.8], np.float32)
    assert run_one(boxes, s, "circle", 1.0).tolist() == [0]         # 1 * 1 + 0 <= 1
    assert run_one(boxes, s, "circle", 0.99).tolist() == [0, 1]
    assert run_one(boxes * 2, s, "circle", 3.99).tolist() == [0, 1]  # distance 2, squared 4: thresh is NOT squared


def test_a_box_layout_with_more_columns_is_read_in_place():
    boxes, scores = scene(129, 5)
    wide = np.zeros((129, 9), np.float32)
    wide[:, :6], wide[:, 6:8], wide[:, 8] = boxes[:, :6], 123.0, boxes[:, 6]
    assert np.array_equal(run_one(wide, scores, "rotate", 0.3), run_one(boxes, scores, "rotate", 0.3))
    assert np.array_equal(run_one(wide, scores, "rotate", 0.3, yaw_col=8), run_one(boxes, scores, "rotate", 0.3))


# ---------------------------------------------------------------------------------- batching, grid, runs
def test_batched_segments_equal_the_single_calls_for_every_grid_and_run():
    rng = np.random.default_rng(3)
    counts = [0] + [int(c) for c in rng.choice([0, 1, 63, 64, 65, 200], 35)] + [0]
    assert len(counts) == 37 and {0, 1, 63, 64, 65, 200} <= set(counts)
    parts = [scene(c, 500 + f) for f, c in enumerate(counts)]
    boxes, scores = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    off = np.concatenate([[0], np.cumsum(counts)])
    b, s = dev(boxes), dev(scores)
    runs = []
    for wg in (0, 3, 0):
        keep, count, order = nms.batched_nms(b, s, off, "rotate", 0.5, 150, 40, max_workgroups=wg, return_order=True)
        assert keep.shape == (37, 40)
        count = count.cpu().numpy()
        live = np.arange(40)[None, :] < count[:, None]
        runs.append((np.where(live, keep.cpu().numpy(), -1), count, order.cpu().numpy()))
    for r in runs[1:]:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(r, runs[0]))
    keep, count, order = runs[0]
    for f, (bx, sc) in enumerate(parts):
        assert np.array_equal(keep[f, :count[f]], run_one(bx, sc, "rotate", 0.5, 150, 40)), f
        assert np.array_equal(order[off[f]:off[f + 1]], nms_ref.order(sc)), f
    # split over two calls
    k0, c0 = nms.batched_nms(b[:off[20]], s[:off[20]], off[:21], "rotate", 0.5, 150, 40)
    k1, c1 = nms.batched_nms(b[off[20]:], s[off[20]:], off[20:] - off[20], "rotate", 0.5, 150, 40)
    assert np.array_equal(np.concatenate([c0.cpu().numpy(), c1.cpu().numpy()]), count)
    both = np.concatenate([k0.cpu().numpy(), k1.cpu().numpy()])
    assert np.array_equal(np.where(np.arange(40)[None, :] < count[:, None], both, -1), keep)


def test_seg_count_limits_the_rows_in_use():
    boxes, scores = scene(200, 9)
    used = torch.tensor([120, 0], dtype=torch.int32, device=DEV)
    keep, count = nms.batched_nms(dev(boxes), dev(scores), [0, 150, 200], "rotate", 0.5, seg_count=used)
    assert int(count[1]) == 0
    assert np.array_equal(keep[0, :int(count[0])].cpu().numpy(), run_one(boxes[:120], scores[:120], "rotate", 0.5))


def test_too_many_candidates_are_reported_on_the_device_or_refused():
    n = hip.NMS_MAX_PRE + 4
    boxes = np.zeros((n, 7), np.float32)
    boxes[:, 0] = np.arange(n) * 10.0
    boxes[:, 3:6] = 1.0
    scores = np.linspace(1.0, 0.0, n).astype(np.float32)
    with pytest.raises(ValueError, match="candidates"):
        nms.batched_nms(dev(boxes), dev(scores), [0, n], "rotate", 0.5)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    keep, count = nms.batched_nms(dev(boxes), dev(scores), [0, 3, n], "rotate", 0.5, 0, 8, status=status)
    assert int(status[0]) == hip.NMS_TOO_MANY and count.cpu().tolist() == [3, 0]
    assert run_one(boxes, scores, "rotate", 0.5, hip.NMS_MAX_PRE, 8).tolist() == list(range(8))   # with the cut it runs


# ---------------------------------------------------------------------------------- the reference's interface
def test_wrappers_return_the_references_types_and_shapes():
    boxes, scores = scene(65, 21)
    b, s = dev(boxes), dev(scores)
    sel, none = nms.nms_gpu(b, s, 0.7, pre_maxsize=50)
    assert none is None and sel.dtype == torch.int64 and sel.dim() == 1 and sel.is_cuda
    assert np.array_equal(sel.cpu().numpy(), host_greedy(boxes, scores, 0.7, 50))
    r = nms.rotate_nms_pcdet(b, s, 0.7, pre_maxsize=50, post_max_size=5)
    assert r.dtype == torch.int64 and r.shape == (5,) and torch.equal(b, dev(boxes))        # the input is not modified
    c = nms.circle_nms(torch.cat([b[:, :2], s[:, None]], 1), 1.0)
    assert c.dtype == torch.int64 and c.dim() == 1 and 0 < c.numel() <= 65
    empty = nms.rotate_nms_pcdet(b[:0], s[:0], 0.7, pre_maxsize=4096, post_max_size=500)
    assert empty.dtype == torch.int64 and empty.shape == (0,)
    with pytest.raises(ValueError):
        nms.nms_gpu(b[:, :6], s, 0.7)
    with pytest.raises(TypeError):
        nms.rotate_nms_pcdet(b.to(torch.float16), s, 0.7)
    with pytest.raises(TypeError, match="host"):
        nms.batched_nms(b, s, torch.tensor([0, 65], device=DEV), "rotate", 0.7)
