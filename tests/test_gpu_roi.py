"""CenterPoint's second stage on the GPU (3dal_pytorch_amd/two_stage.py; dal3_bev_gather, dal3_box_points, dal3_roi_head,
dal3_roi_post): the BEV gather through NCHW and NHWC strides, inside and outside the map and on its discontinuities; the
RoI head's MLP and box prediction through `RoIHead.forward`; the golden case module by module; and the fused `refine` on a
hand-built first-stage result against the modules one by one, bit for bit. Accuracy is held in multiples of the float32
restatement's own error against the float64 truth (roi_ref.BARS); labels, counts, row order and masks exactly."""
import importlib

import numpy as np
import pytest
import torch
from torch import nn

import roi_ref as R
from _common import golden
from roi_gpu import _dev, _hold, _record_file  # noqa: F401

hip = importlib.import_module("3dal_pytorch_amd._hip")
two_stage = importlib.import_module("3dal_pytorch_amd.two_stage")
pytestmark = pytest.mark.gpu

W, H = R.MAP["W"], R.MAP["H"]
EPS32 = 2.0 ** -23


class _First(nn.Module):
    """a stand-in first stage for `refine`, which reads only bbox_head.num_classes"""

    def __init__(self, num_classes):
        super().__init__()
        self.bbox_head = nn.Identity()
        self.bbox_head.num_classes = list(num_classes)


def _detector(head, M, num_classes=(3,), num_point=R.NUM_POINT):
    m = two_stage.TwoStageDetector(_First(num_classes), [dict(type="BEVFeatureExtractor", **R.EXTRACTOR)], head, M, num_point=num_point)
    return m.cuda().eval()


def _head(input_channels, cfg, code, sd):
    head = two_stage.RoIHead(input_channels, cfg, code_size=code)
    head.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    return head.cuda().eval()


def _bev(bev_nhwc, layout):
    """the (B, H, W, C) view BEVFeatureExtractor takes, over NCHW or NHWC storage"""
    t = _dev(bev_nhwc)
    return t.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1) if layout == "NCHW" else t


# ------------------------------------------------------------------------------------- the gather
def _points(tag, n):
    """(near (n, 3), far (8, 3)) absolute points: near ones up to two cells outside every side of the map, none within
    1e-3 cells of the lines 0, W - 1 and H - 1; far ones at +-1e6 m"""
    rel = np.stack([R.synth.uniform(R.SEED, f"{tag}/x", (n,), -2.0, W + 1.0), R.synth.uniform(R.SEED, f"{tag}/y", (n,), -2.0, H + 1.0)], 1)
    for axis, lines in ((0, (0.0, W - 1.0)), (1, (0.0, H - 1.0))):
        for line in lines:
            close = np.abs(rel[:, axis] - line) < 5e-3
            rel[close, axis] += 0.02
    near = np.concatenate([np.asarray(R.EXTRACTOR["pc_start"]) + rel * 0.8, np.zeros((n, 1))], 1).astype(np.float32)
    far = np.asarray([[1e6, 0.3, 0], [-1e6, 0.3, 0], [0.3, 1e6, 0], [0.3, -1e6, 0], [1e6, 1e6, 0], [-1e6, 1e6, 0], [1e6, -1e6, 0],
                      [-1e6, -1e6, 0]], np.float32)
    return near, far


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("C", [1, 20, 64])
def test_gather_inside_outside_and_far(C, layout):
    bev = R.bev_map(f"g{C}", C=C)
    ext = two_stage.BEVFeatureExtractor(**R.EXTRACTOR)
    pts = [_points(f"g{C}/{b}", 300) for b in range(2)]
    for part, name in ((0, "near"), (1, "far")):
        centres = [p[part] for p in pts]
        x, y = R.relative(np.concatenate(centres))
        if name == "near":
            assert min(float((x - l).abs().min()) for l in (0, W - 1)) >= 1e-3 and min(float((y - l).abs().min()) for l in (0, H - 1)) >= 1e-3
            assert (x < 0).any() and (x > W - 1).any() and (y < 0).any() and (y > H - 1).any() and ((x > 0) & (x < W - 1)).any()
        got = ext({"bev_feature": _bev(bev, layout)}, [_dev(c) for c in centres], 1)
        assert [tuple(g.shape) for g in got] == [(c.shape[0], C) for c in centres]
        truth, f32 = R.bev_features(bev, centres, 1, dtype=R.F64), R.bev_features(bev, centres, 1, dtype=R.F32)
        if name == "near":
            _hold(f"gather/{name}/c{C}/{layout}", torch.cat(got), torch.cat(f32), torch.cat(truth))
            continue
        # +-1e6 m: the definition gives 0 * I there, four products of ~1e6 (~1e12 with both coordinates far) times I that
        # cancel. In float64 they cancel to ~1e-10 or exactly, in float32 they leave the rounding of their sums, so a
        # ratio to the truth says nothing. Held instead: finite, and no larger than the rounding of those sums, 8 ulp of
        # the largest product |I| (|x| + W) (|y| + H)
        g = torch.cat(got).cpu().numpy()
        bound = 8 * EPS32 * float(bev.max()) * ((x.abs() + W) * (y.abs() + H)).numpy()
        same = np.array_equal(g, torch.cat(f32).numpy())
        print(f"gather/far/c{C}/{layout}: max |got| {np.abs(g).max():.3e}, the smallest bound {bound.min():.3e}, float32 restatement's bits "
              f"{'equal' if same else 'differ'}")
        assert np.isfinite(g).all() and (np.abs(g) <= bound[:, None]).all()


def _abs_for(rel_target, axis):
    """an absolute float32 coordinate whose float32 relative coordinate is exactly rel_target"""
    start, cell = np.float32(R.EXTRACTOR["pc_start"][axis]), 0.8
    a = np.float32(float(start) + float(rel_target) * cell)

    def rel(v):
        return (v - start) / np.float32(R.EXTRACTOR["voxel_size"][axis]) / np.float32(R.EXTRACTOR["out_stride"])
    for _ in range(64):
        r = rel(a)
        if r == rel_target:
            return a
        a = np.nextafter(a, np.float32(np.inf if r < rel_target else -np.inf))
    raise AssertionError(f"no float32 coordinate maps to {rel_target!r}")


@pytest.mark.parametrize("axis", [0, 1])
def test_gather_on_the_lines_themselves(axis):
    """the centre point (its coordinate arithmetic is three IEEE operations, bit-reproducible) exactly on the line
    x = W - 1 (y = H - 1), one ulp below and one ulp above it, the other coordinate exactly on an interior cell line (so
    that the four products cancel exactly): on and above the line the output is exactly zero, below it it is the
    interpolation, within the bar of the float32 restatement"""
    C = 20
    bev = R.bev_map("line", C=C)
    line = np.float32((W - 1) if axis == 0 else (H - 1))
    other = _abs_for(np.float32(3.0 if axis == 0 else 2.0), 1 - axis)
    rels = [np.nextafter(line, np.float32(0)), line, np.nextafter(line, np.float32(np.inf))]
    pts = np.zeros((3, 3), np.float32)
    pts[:, axis] = [_abs_for(r, axis) for r in rels]
    pts[:, 1 - axis] = other
    x, y = R.relative(pts, dtype=R.F32)
    assert list((x if axis == 0 else y).numpy()) == rels
    ext = two_stage.BEVFeatureExtractor(**R.EXTRACTOR)
    f32 = torch.cat(R.bev_features(bev, [pts, pts], 1, dtype=R.F32)).numpy()
    for layout in ("NCHW", "NHWC"):
        got = torch.cat(ext({"bev_feature": _bev(bev, layout)}, [_dev(pts), _dev(pts)], 1)).cpu().numpy()
        for b in range(2):
            below, on, above = got[3 * b], got[3 * b + 1], got[3 * b + 2]
            assert not f32[3 * b + 1].any() and not f32[3 * b + 2].any() and f32[3 * b].any()
            assert not on.any() and not above.any()
            print(f"line axis {axis} {layout} sample {b}: below the line max |got - f32| {np.abs(below - f32[3 * b]).max():.3e}")
            assert np.abs(below - f32[3 * b]).max() <= R.BARS["tensor"] * EPS32 * np.abs(f32[3 * b]).max()


def test_gather_of_an_impulse_pins_taps_and_weights():
    bev = np.zeros((2, H, W, 20), np.float32)
    bev[1, 2, 5, 3] = 1.0
    rel = np.asarray([[5.25, 2.5], [4.25, 2.5], [5.0, 2.0], [4.75, 1.125], [5.5, 3.5], [6.5, 2.0], [3.5, 2.0], [5.0, 0.5]])
    pts = np.concatenate([np.asarray(R.EXTRACTOR["pc_start"]) + rel * 0.8, np.zeros((8, 1))], 1).astype(np.float32)
    ext = two_stage.BEVFeatureExtractor(**R.EXTRACTOR)
    truth = torch.cat(R.bev_features(bev, [pts, pts], 1)).numpy()
    for layout in ("NCHW", "NHWC"):
        got = torch.cat(ext({"bev_feature": _bev(bev, layout)}, [_dev(pts), _dev(pts)], 1)).cpu().numpy()
        assert not got[:8].any()                                             # sample 0 is empty
        assert np.array_equal(got != 0, np.abs(truth) > 1e-5)
        assert (got[:, np.arange(20) != 3] == 0).all()
        want = np.asarray([0.75 * 0.5, 0.25 * 0.5, 1.0, 0.75 * 0.125, 0.0, 0.0, 0.0, 0.0])
        assert np.abs(got[8:, 3] - want).max() < 4e-6 and np.abs(got - truth).max() < 4e-6


# ------------------------------------------------------------------------------------- the MLP and the box prediction
def _head_case(tag, M, code, cfg, c_in):
    feats = np.maximum(R.synth.uniform(R.SEED, f"{tag}/f", (1, M, c_in), -0.5, 2.0), 0.0).astype(np.float32)
    rois = R.boxes(f"{tag}/rois", M, code)
    if code == 9:
        rois = rois[:, [0, 1, 2, 3, 4, 5, 8, 6, 7]]
    assert M < 8 or (np.abs(rois[:, 6]) > np.pi).any()                        # headings beyond +-pi
    scores = R.synth.uniform(R.SEED, f"{tag}/s", (1, M), 0.1, 0.95).astype(np.float32)
    return dict(sd=R.head_weights(c_in, cfg, code, tag), cfg=cfg, rois=rois[None], roi_scores=scores, roi_features=feats)


def _run_head(case, code):
    head = _head(case["roi_features"].shape[-1], case["cfg"], code, case["sd"])
    d = {k: _dev(case[k]) for k in ("rois", "roi_scores", "roi_features")}
    out = head(d, training=False)
    assert out is d and out["cls_preds_normalized"] is False and out["batch_size"] == case["rois"].shape[0]
    return out["batch_cls_preds"], out["batch_box_preds"]


@pytest.mark.parametrize("code", [7, 9])
@pytest.mark.parametrize("M", [1, 37, 500])
def test_roi_head_forward(M, code):
    case = _head_case(f"mlp{M}c{code}", M, code, R.SMALL, 100)
    cls, box = _run_head(case, code)
    assert tuple(cls.shape) == (1, M, 1) and tuple(box.shape) == (1, M, code)
    (tc, tb), (yc, yb) = R.head_alone(case, R.F64), R.head_alone(case, R.F32)
    if M > 1:
        _hold(f"head/cls/m{M}/c{code}", cls, yc, tc)
        _hold(f"head/box/m{M}/c{code}", box, yb, tb)
    else:
        # one row: every measure is one rounding error over another, which can be zero. The row is held to 64 ulp of the
        # largest value instead (sums of at most 100 terms of like size: sqrt(100) x a few ulp each, four layers deep)
        for got, want in ((cls, tc), (box, tb)):
            d = np.abs(got.cpu().numpy().astype(np.float64) - want.numpy())
            print(f"head/m1/c{code}: max |d| {d.max():.3e}, max |truth| {np.abs(want.numpy()).max():.3e}")
            assert d.max() <= 64 * EPS32 * max(1.0, float(np.abs(want.numpy()).max()))


def test_roi_head_at_the_production_widths():
    g, case = golden("roi"), R.production_case()
    cls, box = _run_head(case, 9)
    for name, got in (("cls", cls), ("box_preds", box)):
        f32 = g[f"prod_{name}_f32"]
        _hold(f"head/prod/{name}", got, f32, f32.astype(np.float64) + g[f"prod_{name}_diff"].astype(np.float64))


def test_pack_is_fold_bit_for_bit():
    """dal3_roi_pack's buffer, read back: per layer the folded bias of every GEMM row, then the fragments
    [out tile][8 inputs][lane] float4 with element e of a lane = W'[32 tile + lane % 32][8 c8 + 2 e + lane // 32], zeros
    beyond the layer's rows and inputs; W' and b' are roi_ref.fold's bits"""
    case = R.golden_case(9)
    sd, head = case["sd"], _head(100, case["cfg"], 9, case["sd"])
    packed = head.packed().cpu().numpy()
    at = 0
    for conv, bn, _ in R.layer_names(case["cfg"]):
        wf, bf = R.fold(sd[conv + "weight"], sd.get(conv + "bias"), None if bn is None else R.bn_of(sd, bn), 1e-5)
        c_out, c_in = wf.shape
        tiles, nc8 = -(-c_out // 32), -(-c_in // 8)
        bias = np.zeros(tiles * 32, np.float32)
        bias[:c_out] = bf
        assert np.array_equal(packed[at:at + tiles * 32].view(np.uint32), bias.view(np.uint32)), conv
        at += tiles * 32
        full = np.zeros((tiles * 32, nc8 * 8), np.float32)
        full[:c_out, :c_in] = wf
        ot, c8, lane, e = np.meshgrid(np.arange(tiles), np.arange(nc8), np.arange(64), np.arange(4), indexing="ij")
        want = full[32 * ot + lane % 32, 8 * c8 + 2 * e + lane // 32]
        got = packed[at:at + want.size].reshape(want.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), conv
        at += want.size
    assert at == packed.size


@pytest.mark.parametrize("code", [7, 9])
def test_golden_case_module_by_module(code):
    """the reference's own outputs (tests/golden/roi.npz): get_box_center -> BEVFeatureExtractor -> reorder -> RoIHead ->
    post_process on the device, each stage held against the reference's .double() run"""
    g, tag, case = golden("roi"), f"c{code}", R.golden_case(code)
    m = _detector(_head(100, case["cfg"], code, case["sd"]), R.GOLDEN_M)
    first = [{"box3d_lidar": _dev(p["box3d_lidar"]), "scores": _dev(p["scores"]), "label_preds": _dev(p["label_preds"])}
             for p in case["pred"]]

    def truth(name):
        return g[f"{tag}_{name}_f32"].astype(np.float64) + g[f"{tag}_{name}_diff"].astype(np.float64)
    centres = m.get_box_center(first)
    x, y = R.relative(truth("centres"))
    assert min(float((x - l).abs().min()) for l in (0, W - 1)) >= 1e-3 and min(float((y - l).abs().min()) for l in (0, H - 1)) >= 1e-3
    _hold(f"golden/{tag}/centres", torch.cat(centres), g[f"{tag}_centres_f32"], truth("centres"))
    feats = m.second_stage[0]({"bev_feature": _dev(case["bev"])}, centres, R.NUM_POINT)
    _hold(f"golden/{tag}/features", torch.cat(feats), g[f"{tag}_features_f32"], truth("features"))
    example = m.reorder_first_stage_pred_and_feature(first, {"metadata": [None, None]}, [feats])
    out = m.roi_head(example, training=False)
    _hold(f"golden/{tag}/cls", out["batch_cls_preds"], g[f"{tag}_cls_f32"], truth("cls"))
    _hold(f"golden/{tag}/box_preds", out["batch_box_preds"], g[f"{tag}_box_preds_f32"], truth("box_preds"))
    final = m.post_process(out)
    assert [int(f["scores"].numel()) for f in final] == list(R.GOLDEN_BOXES)
    labels = torch.cat([f["label_preds"] for f in final])
    assert labels.dtype == torch.int64 and np.array_equal(labels.cpu().numpy(), g[f"{tag}_final_labels"])
    _hold(f"golden/{tag}/final_boxes", torch.cat([f["box3d_lidar"] for f in final]), g[f"{tag}_final_boxes_f32"], truth("final_boxes"))
    _hold(f"golden/{tag}/final_scores", torch.cat([f["scores"] for f in final]), g[f"{tag}_final_scores_f32"], truth("final_scores"))


# ------------------------------------------------------------------------------------- the fused route
SEG_ROWS, T, B = 16, 2, 3
NUM_CLASSES = (1, 2)


def _first_stage_result(code, counts):
    """a decode_nms dictionary built by hand: T = 2 tasks, B = 3 samples, 16 rows a segment, the kept rows out of order
    within their segments; counts[t][b] rows kept"""
    F, K = T * B, T * B * SEG_ROWS
    keep = np.stack([np.argsort(R.synth.uniform(R.SEED, f"fused/keep/{f}", (SEG_ROWS,))) for f in range(F)]).astype(np.int32)
    assert sum(bool((np.diff(keep[f][:4]) < 0).any()) for f in range(F)) >= 4          # out of order within the segments
    off = np.arange(F + 1, dtype=np.int64) * SEG_ROWS
    labels = np.concatenate([(R.synth.uniform(R.SEED, f"fused/l/{f}", (SEG_ROWS,), 0, 8).astype(np.int32) % NUM_CLASSES[f // B])
                             for f in range(F)])
    return {"boxes": _dev(R.boxes("fused/boxes", K, code)), "scores": _dev(R.synth.uniform(R.SEED, "fused/s", (K,), 0.1, 0.95).astype(np.float32)),
            "labels": _dev(labels), "keep": _dev(keep), "keep_count": _dev(np.asarray(counts, np.int32).reshape(-1)),
            "seg_offsets": off, "seg_offsets_device": _dev(off), "status": torch.zeros(1, dtype=torch.int32).cuda(), "B": B}


def _first_list(r, M):
    """CenterHeadPost.predict's list from the dictionary (tasks in order, keep order within a task), cut at M rows"""
    count, out = r["keep_count"].cpu().numpy(), []
    for b in range(B):
        rows, labels = [], []
        for t in range(T):
            f = t * B + b
            rows.append(r["keep"][f, :int(count[f])].long() + int(r["seg_offsets"][f]))
            labels.append(r["labels"][rows[-1]].long() + sum(NUM_CLASSES[:t]))
        rows, labels = torch.cat(rows)[:M], torch.cat(labels)[:M]
        out.append({"box3d_lidar": r["boxes"][rows], "scores": r["scores"][rows], "label_preds": labels})
    return out


@pytest.mark.parametrize("M,code", [(1, 7), (11, 9), (11, 7)])
def test_refine_equals_the_modules_one_by_one(M, code):
    # sample 0 keeps nothing, sample 1 exactly M rows, sample 2 M + 1 (then M - 1 in the second run)
    counts = {1: [[0, 0, 1], [0, 1, 1]], 11: [[0, 4, 5], [0, 7, 7]]}[M]
    case = R.golden_case(code)
    m = _detector(_head(100, case["cfg"], code, case["sd"]), M, NUM_CLASSES)
    bev = _dev(R.bev_map("fused", B=B)).permute(0, 3, 1, 2).contiguous()      # the neck's NCHW map
    for overflow in (True, False):
        c = [list(row) for row in counts]
        if not overflow:
            c[1][2] -= 2 if M > 1 else 1
        r = _first_stage_result(code, c)
        kept = [c[0][b] + c[1][b] for b in range(B)]
        m.refine(r, bev)                                                       # warm: the pack
        r["status"].zero_()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = m.refine(r, bev)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert out["status"] is r["status"] and int(out["status"].item()) == (hip.ROI_OVERFLOW if overflow else 0)
        assert out["counts"].dtype == torch.int32 and out["counts"].tolist() == [min(k, M) for k in kept]
        assert tuple(out["boxes"].shape) == (B, M, code) and out["labels"].dtype == torch.int32
        # ---- the modules one by one on the same rows
        first = _first_list(r, M)
        centres = m.get_box_center(first)
        feats = m.second_stage[0]({"bev_feature": bev.permute(0, 2, 3, 1)}, centres, R.NUM_POINT)
        example = m.reorder_first_stage_pred_and_feature(first, {"metadata": [None] * B}, [feats])
        final = m.post_process(m.roi_head(example, training=False))
        for b in range(B):
            n = min(kept[b], M)
            assert torch.equal(out["features"][b, :n], feats[b]) and not out["features"][b, n:].any()
            assert torch.equal(out["boxes"][b, :n], final[b]["box3d_lidar"]) and not out["boxes"][b, n:].any()
            assert torch.equal(out["scores"][b, :n], final[b]["scores"]) and not out["scores"][b, n:].any()
            assert torch.equal(out["labels"][b, :n].long(), final[b]["label_preds"]) and final[b]["label_preds"].dtype == torch.int64
        assert int(final[1]["scores"].numel()) == M and bool((final[1]["scores"] > 0).all())
        if overflow:
            with pytest.raises(RuntimeError, match="NMS_POST_MAXSIZE"):
                m._finish(out, None)
        else:
            got = m._finish(out, [{"token": str(b)} for b in range(B)])
            for b in range(B):
                assert torch.equal(got[b]["box3d_lidar"], final[b]["box3d_lidar"]) and torch.equal(got[b]["label_preds"], final[b]["label_preds"])
                assert got[b]["label_preds"].dtype == torch.int64 and got[b]["metadata"] == {"token": str(b)}


def test_refine_refuses_what_does_not_fit():
    case = R.golden_case(9)
    m = _detector(_head(100, case["cfg"], 9, case["sd"]), 11, NUM_CLASSES)
    r = _first_stage_result(7, [[0, 1, 1], [0, 1, 1]])
    with pytest.raises(ValueError, match="code_size"):
        m.refine(r, torch.zeros((B, 20, H, W)).cuda())
    with pytest.raises(ValueError, match="input channels"):
        m.refine(_first_stage_result(9, [[0, 1, 1], [0, 1, 1]]), torch.zeros((B, 24, H, W)).cuda())
