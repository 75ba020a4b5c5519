"""The training run on the MI355X: the fused box-estimation metric kernel (metrics.py, dal3_box_estimation_metrics)
against iou.paired_iou on the NumPy decode and against host counts, and the file-level run (fit.py) on a synthetic
segment: log lines, checkpoints, per-epoch numbers against a host recomputation of the recorded steps, the batch
order, the first step against a hand-written reference-shaped step, and no device->host read per step."""
import importlib
import pickle
import re

import numpy as np
import pytest
import torch
from torch.utils.data import RandomSampler

from _common import synth

metrics = importlib.import_module("3dal_pytorch_amd.metrics")
iou = importlib.import_module("3dal_pytorch_amd.iou")
fit = importlib.import_module("3dal_pytorch_amd.fit")
ev = importlib.import_module("3dal_pytorch_amd.eval")
static_model = importlib.import_module("3dal_pytorch_amd.static_model")
dynamic_model = importlib.import_module("3dal_pytorch_amd.dynamic_model")
pytestmark = pytest.mark.gpu
DEV = "cuda"
THR = np.float32(0.7)


def _batch(B, seed, two=False):
    """head-shaped outputs with the per-item fields as views of a (B, 39) box_pred, and prep-shaped labels"""
    g = torch.Generator().manual_seed(seed)
    bp = torch.randn(B, 39, generator=g)
    bp[: B // 4, 3:15] = 0.5                                        # all heading scores tied
    bp[B // 4: B // 2, 27:30] = 1.0                                 # all size scores tied
    bp = bp.to(DEV)
    hr = (torch.randn(B, 12, generator=g) * 0.3).to(DEV)
    sr = (torch.randn(B, 3, 3, generator=g) * 0.3).to(DEV)
    # centres near the labels' so that many pairs overlap
    cl = torch.randn(B, 3, generator=g).double()
    out = {"center": bp[:, 0:3], "heading_scores": bp[:, 3:15], "heading_residuals": hr, "size_scores": bp[:, 27:30],
           "size_residuals": sr}
    bp[:, 0:3] = (cl + 0.3 * torch.randn(B, 3, generator=g, dtype=torch.float64)).float().to(DEV)
    bp[3 * B // 4:, 0] += 20.0                                      # disjoint pairs: an exact 0
    lab = {"center_label": cl.to(DEV), "heading_class_label": torch.randint(0, 12, (B,), generator=g).to(DEV),
           "heading_residuals_label": (torch.randn(B, generator=g, dtype=torch.float64) * 0.2).to(DEV),
           "size_class_label": torch.randint(0, 3, (B,), generator=g).to(DEV),
           "size_residual_label": (torch.randn(B, 3, generator=g, dtype=torch.float64) * 0.3).to(DEV)}
    hc = torch.argmax(bp[:, 3:15], 1)
    lab["heading_class_label"][: B // 3] = hc[: B // 3]             # same heading bin: high IoU items
    near = slice(B // 2, B // 2 + B // 8 + 1)                       # near-copies of the prediction: IoU above 0.7
    sc, ar = torch.argmax(bp[:, 27:30], 1), torch.arange(B, device=DEV)
    lab["center_label"][near] = bp[near, 0:3].double() + 0.01
    lab["heading_class_label"][near] = hc[near]
    lab["heading_residuals_label"][near] = hr[ar, hc][near].double()
    lab["size_class_label"][near] = sc[near]
    lab["size_residual_label"][near] = sr[ar, sc][near].double()
    if two:
        out["heading_class_label_two"] = torch.randint(0, 12, (B,), generator=g).to(DEV)
        out["heading_residuals_label_two"] = (torch.randn(B, generator=g) * 0.2).to(DEV)
    return out, lab


def _host_boxes(out, lab, two=False):
    c = {k: v.cpu().numpy() for k, v in out.items()}
    hcl = c["heading_class_label_two"] if two else lab["heading_class_label"].cpu().numpy()
    hrl = c["heading_residuals_label_two"] if two else lab["heading_residuals_label"].cpu().numpy()
    return metrics.decode_boxes_numpy(c["center"], c["heading_scores"], c["heading_residuals"], c["size_scores"],
                                      c["size_residuals"], lab["center_label"].cpu().numpy(), hcl, hrl,
                                      lab["size_class_label"].cpu().numpy(), lab["size_residual_label"].cpu().numpy())


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("B", [0, 1, 65, 4096])
def test_per_item_iou_is_paired_iou_of_the_numpy_decode(B, two):
    out, lab = _batch(B, 10 + B, two)
    vb, v3 = metrics.box_estimation_iou(out, lab, two_stage=two)
    pred, label = _host_boxes(out, lab, two)
    wb, w3 = iou.paired_iou(torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV))
    assert vb.shape == (B,) and vb.dtype == torch.float32
    assert torch.equal(vb, wb) and torch.equal(v3, w3)
    if B > 64:
        assert (v3 > 0.5).any() and (v3 == 0).any()
    dense = {k: v.contiguous() for k, v in out.items()}             # the views and contiguous copies: the same bits
    assert out["heading_scores"].stride(0) == 39
    cb, c3 = metrics.box_estimation_iou(dense, lab, two_stage=two)
    assert torch.equal(cb, vb) and torch.equal(c3, v3)


def test_out_of_range_class_labels_give_nan_and_nan_scores_pick_the_first_nan():
    out, lab = _batch(8, 3)
    lab["heading_class_label"][:2] = torch.tensor([-1, 12], device=DEV)
    lab["size_class_label"][2] = 7
    out["heading_scores"][3, 5] = float("nan")
    vb, v3 = metrics.box_estimation_iou(out, lab)
    assert torch.isnan(vb[:3]).all() and torch.isnan(v3[:3]).all() and torch.isfinite(v3[3:]).all()
    pred, _ = _host_boxes(out, lab)
    assert pred[3, 6] == 5 * (2 * np.pi / 12) + float(out["heading_residuals"][3, 5]) or \
        pred[3, 6] == 5 * (2 * np.pi / 12) + float(out["heading_residuals"][3, 5]) - 2 * np.pi


def _logits(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(B, 2, N, generator=g)                          # (B, N, 2) as a strided view
    lg[:, 1, ::7] = lg[:, 0, ::7]                                    # ties: class 0
    lg[:, 0, 3::11] = float("nan")                                  # NaN is the maximum
    lg[:, 1, 5::13] = float("nan")
    lg[0, :, 9] = float("nan")
    mask = (torch.rand(B, N, generator=g) > 0.5).to(torch.uint8)
    return lg.to(DEV).transpose(1, 2), mask.to(DEV)


@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.bool, torch.float32])
@pytest.mark.parametrize("B,N", [(3, 1000), (5, 4096), (2, 5120)])
def test_segmentation_count_equals_torch_argmax(B, N, mask_dtype):
    logits, mask = _logits(B, N, B * N)
    mask = mask.to(mask_dtype)
    out, lab = _batch(B, 7)
    out["logits"], lab["mask_label"] = logits, mask
    m = metrics.TrainMetrics(DEV, N)
    m.update(out, lab)
    want = int((torch.argmax(logits, 2) == mask.long()).sum())
    c = m.counts()
    assert c["n_seg_correct"] == want and c["n_samples"] == B
    assert logits.stride() == (2 * N, 1, N)


def test_accumulator_counts_sums_and_reproducibility():
    def run():
        m = metrics.TrainMetrics(DEV, 512)
        host = {"bev": [], "v3": [], "seg": 0, "loss": 0.0, "n": 0}
        for k, B in enumerate((64, 1, 300)):
            out, lab = _batch(B, 100 + k)
            out["logits"], lab["mask_label"] = _logits(B, 512, k)
            loss = torch.tensor(0.37 * (k + 1), device=DEV)
            m.update(out, lab, loss)
            pred, label = _host_boxes(out, lab)
            wb, w3 = iou.paired_iou(torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV))
            host["bev"].append(wb.cpu().numpy())
            host["v3"].append(w3.cpu().numpy())
            host["seg"] += int((torch.argmax(out["logits"], 2) == lab["mask_label"].long()).sum())
            host["loss"] += float(loss)
            host["n"] += B
        return m, host
    m1, host = run()
    m2, _ = run()
    assert torch.equal(m1.acc, m2.acc)                              # bit-identical accumulators
    c = m1.result()
    bev, v3 = np.concatenate(host["bev"]), np.concatenate(host["v3"])
    assert c["n_samples"] == host["n"] and c["n_seg_correct"] == host["seg"]
    assert c["n_iou_3d_pass"] == int(np.sum(v3 >= THR)) > 0
    for got, want in ((c["sum_iou_bev"], np.sum(bev, dtype=np.float64)), (c["sum_iou_3d"], np.sum(v3, dtype=np.float64)),
                      (c["sum_loss"], host["loss"])):
        assert abs(got - want) <= 1e-12 * abs(want)
    assert c["seg_acc"] == host["seg"] / (host["n"] * 512.0) and c["iou3d_acc"] == c["n_iou_3d_pass"] / host["n"]


def test_compute_box3d_iou_host_signature():
    out, lab = _batch(65, 5)
    vb, v3 = metrics.box_estimation_iou(out, lab)
    c = {k: v.cpu().numpy() for k, v in out.items()}
    lb = {k: v.cpu().numpy() for k, v in lab.items()}
    hb, h3 = metrics.compute_box3d_iou(c["center"], c["heading_scores"], c["heading_residuals"], c["size_scores"],
                                       c["size_residuals"], lb["center_label"], lb["heading_class_label"],
                                       lb["heading_residuals_label"], lb["size_class_label"], lb["size_residual_label"])
    assert hb.dtype == np.float32 and h3.dtype == np.float32
    assert np.array_equal(hb, vb.cpu().numpy()) and np.array_equal(h3, v3.cpu().numpy())


# ------------------------------------------------------------------ the file-level run
def _segment(tmp_path, head, split=2):
    paths, tracks, poses, dets, has_gt = synth.segment_files(str(tmp_path), 91, n_frames=10, n_tracks=13)
    with open(paths[head], "rb") as f:
        track = pickle.load(f)
    keys = list(track)
    name = "trackStatic" if head == "static" else "trackDynamic"
    for i in range(split):
        with open(tmp_path / f"{name}_{i}.pkl", "wb") as f:
            pickle.dump({k: track[k] for k in keys[i::split]}, f)
    return paths


_TRAIN_LINES = [r"=== Epoch \[{e}/{n}\] ===", r"\[Train\] loss: [-\d.naninf]+, seg acc: [\d.nan]+",
                r"\[Train\] Box IoU \(2D/3D\): [\d.nan]+/[\d.nan]+", r"\[Train\] Box estimation accuracy \(IoU=0.7\): [\d.nan]+",
                r"\[Eval\] loss: [-\d.naninf]+, seg acc: [\d.nan]+", r"\[Eval\] Box IoU \(2D/3D\): [\d.nan]+/[\d.nan]+",
                r"\[Eval\] Box estimation accuracy \(IoU=0.7\): [\d.nan]+"]


def _host_numbers(steps, n_points, two):
    n = sum(len(s["idx"]) for s in steps)
    loss = sum(s["loss"] for s in steps)
    seg = sum(s["seg"] for s in steps)
    bev = np.concatenate([s["bev"] for s in steps]).astype(np.float64)
    v3 = np.concatenate([s["v3"] for s in steps])
    return {"n": n, "loss": loss / n, "seg": seg, "seg_acc": seg / (n * float(n_points)), "iou2d": bev.sum() / n,
            "iou3d": v3.astype(np.float64).sum() / n, "n_pass": int(np.sum(v3 >= THR))}


def _recorder(two):
    steps = []

    def rec(r):
        out, lab = r["output"], r["labels"]
        c = {k: out[k].detach() for k in ("center", "heading_scores", "heading_residuals", "size_scores", "size_residuals")}
        if two:
            c["heading_class_label_two"], c["heading_residuals_label_two"] = out["heading_class_label_two"], out["heading_residuals_label_two"]
        pred, label = _host_boxes(c, lab, two)
        wb, w3 = iou.paired_iou(torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV))
        seg = int((torch.argmax(out["logits"].detach(), 2) == lab["mask_label"].long()).sum())
        steps.append({"idx": list(r["idx"]), "loss": float(r["loss"].detach()), "seg": seg, "bev": wb.cpu().numpy(),
                      "v3": w3.cpu().numpy()})
    return steps, rec


def _batch_size(tmp_path, paths, head):
    """a batch size of 3 to 5 whose last training batch is not a single item: BatchNorm's batch statistics (the heads'
    FC tails) need two rows, in the reference as here"""
    ev.fix_seed(fit.SEED)
    annos = ev.Annos(ev.reorganize_info(pickle.load(open(paths["infos"], "rb"))))
    tr, _ = fit.split_tracks(fit.load_tracks(str(tmp_path), head, 2), annos if head == "static" else None)
    n = len(tr) if head == "static" else len(ev._dynamic_items(tr, annos))
    return next(bs for bs in (3, 4, 5) if n % bs != 1)


def _close(a, b, tol=1e-6):
    return abs(a - b) <= tol * max(abs(b), 1e-30)


@pytest.mark.parametrize("head,model_type", [("static", "one_box_est"), ("static", "two_box_est"), ("dynamic", None)])
def test_fit_run_end_to_end(tmp_path, monkeypatch, head, model_type):
    paths = _segment(tmp_path, head)
    two = model_type == "two_box_est"
    n_points = metrics.NUM_POINT_STATIC if head == "static" else metrics.NUM_POINT_DYNAMIC * metrics.NUM_FRAME
    train_steps, rec_train = _recorder(two)
    eval_steps, rec_eval = _recorder(two)
    orders = []
    orig_loader = fit.loader

    def loader(n, batch_size, shuffle):
        if shuffle:
            orders.append((torch.get_rng_state(), n))
        return orig_loader(n, batch_size, shuffle)
    monkeypatch.setattr(fit, "loader", loader)
    hist = fit.run(head, str(tmp_path), paths["infos"], model_type or "one_box_est", split=2, n_epoch=2,
                   batch_size=_batch_size(tmp_path, paths, head), on_train_step=rec_train, on_eval_step=rec_eval)
    assert len(hist) == 2
    # per-epoch numbers against the recorded steps
    per_epoch_train = len(train_steps) // 2
    per_epoch_eval = len(eval_steps) // 2
    for e, h in enumerate(hist):
        for got, steps in ((h["train"], train_steps[e * per_epoch_train:(e + 1) * per_epoch_train]),
                           (h["eval"], eval_steps[e * per_epoch_eval:(e + 1) * per_epoch_eval])):
            want = _host_numbers(steps, n_points, two)
            assert got["n_samples"] == want["n"] > 0
            assert got["n_seg_correct"] == want["seg"] and got["n_iou_3d_pass"] == want["n_pass"]
            for k in ("loss", "seg_acc", "iou2d", "iou3d"):
                assert _close(got[k], want[k]), (e, k, got[k], want[k])
            assert got["iou3d_acc"] == want["n_pass"] / want["n"]
    # batch order: a replay of DataLoader(shuffle=True)'s RandomSampler from the same torch state
    assert len(orders) == 2
    for e, (state, n) in enumerate(orders):
        keep = torch.get_rng_state()
        torch.set_rng_state(state)
        torch.empty((), dtype=torch.int64).random_()               # the loader iterator's base seed
        want = list(RandomSampler(range(n)))
        torch.set_rng_state(keep)
        got = [k for s in train_steps[e * per_epoch_train:(e + 1) * per_epoch_train] for k in s["idx"]]
        if head == "static":
            assert got == want
        else:                                                        # the numpy sampler may substitute items
            assert len(got) == len(want)
    # log lines and checkpoints
    root = tmp_path / head
    log = root / "log" / "train" / (f"{model_type}.txt" if head == "static" else "train.txt")
    lines = [re.sub(r"^\S+ \S+\s+INFO\s+", "", ln) for ln in log.read_text().splitlines()]
    assert lines[:3] == ["Load track data", "Load info data", "Start training"]
    k = 3
    result_dir = root / "model" / model_type if head == "static" else root / "model"
    for e, h in enumerate(hist):
        for pat in _TRAIN_LINES:
            assert re.fullmatch(pat.format(e=e + 1, n=2), lines[k]), (lines[k], pat)
            k += 1
        if h["saved"] is not None:
            assert lines[k] == f"Model save to {h['saved']}"
            assert h["saved"].name == f"acc{h['eval']['iou3d_acc']:04f}_epoch{e + 1:03d}.pth"
            k += 1
    saved = [h["saved"] for h in hist if h["saved"] is not None]
    assert saved, "no checkpoint: every eval accuracy was nan"
    best_acc = max(h["eval"]["iou3d_acc"] for h in hist)
    best = result_dir / f"acc{best_acc:04f}_best.pth"
    assert lines[k] == f"Model save to {saved[-1] if head == 'static' else best}"
    assert lines[k + 1:] == ["Done."]
    assert sorted(p.name for p in result_dir.iterdir()) == sorted([p.name for p in saved] + [best.name])
    ckpt = torch.load(best, map_location="cpu")
    assert set(ckpt) == {"epoch", "train_iou3d_acc", "eval_iou3d_acc", "model_state_dict", "optimizer_state_dict"}
    fresh = (static_model.StaticModelOneBoxEst if model_type == "one_box_est" else static_model.StaticModelTwoBoxEst
             if head == "static" else dynamic_model.DynamicModel)(n_classes=3, n_channel=3 if head == "static" else 4)
    fresh.load_state_dict(ckpt["model_state_dict"], strict=True)
    final, _ = ev.run(head, paths[head], paths["infos"], paths["det_annos"], str(best), model_type or "one_box_est",
                      batch_size=4, sampler="device")
    assert np.isfinite(final).all()


def _cuda_reads(monkeypatch):
    """count device->host reads of CUDA tensors (item / cpu / numpy / tolist and the Python conversions)"""
    n = {"reads": 0, "on": True}
    for name in ("item", "cpu", "numpy", "tolist", "__float__", "__int__", "__bool__", "__index__"):
        orig = getattr(torch.Tensor, name)

        def wrap(self, *a, _orig=orig, **k):
            if n["on"] and self.is_cuda:
                n["reads"] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, wrap)
    return n


def test_no_device_read_per_step(tmp_path, monkeypatch):
    paths = synth.segment_files(str(tmp_path), 92, n_frames=6, n_tracks=18)[0]
    with open(paths["static"], "rb") as f:
        track = pickle.load(f)
    infos = ev.reorganize_info(pickle.load(open(paths["infos"], "rb")))
    annos = ev.Annos(infos)
    track = ev.preprocessing(track, annos)
    keys = list(track)
    assert len(keys) >= 12
    counts = {}
    n = _cuda_reads(monkeypatch)
    orig_batch = fit.StaticBatches.batch

    def batch(self, *a, **k):                                       # prep is outside the count
        n["on"] = False
        try:
            return orig_batch(self, *a, **k)
        finally:
            n["on"] = True
    monkeypatch.setattr(fit.StaticBatches, "batch", batch)
    for steps in (2, 6):
        data = fit.StaticBatches({k: track[k] for k in keys[:2 * steps]}, annos, n_points=1024, sampler="device")
        torch.manual_seed(1)
        model = static_model.StaticModelOneBoxEst().to(DEV)
        model.sampler = "device"
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        n["reads"] = 0
        m, drawn = fit.train_one_epoch(model, data, static_model.FrustumPointNetLossOneBoxEst(), opt, 2, 1024, False)
        counts[steps] = n["reads"]
        assert drawn == 2 * steps
        assert m.result()["n_samples"] == 2 * steps
    assert counts[2] == counts[6], counts


def test_first_step_equals_a_reference_shaped_step(tmp_path, monkeypatch):
    paths = _segment(tmp_path, "static")
    states, first = [], {}
    orig_batch = fit.StaticBatches.batch

    def batch(self, *a, **k):
        out = orig_batch(self, *a, **k)
        states.append((torch.get_rng_state(), np.random.get_state()))
        return out
    monkeypatch.setattr(fit.StaticBatches, "batch", batch)

    def rec(r):
        if not first:
            first["inputs"] = [t.detach().clone() for t in r["inputs"]]
            first["labels"] = {k: v.clone() for k, v in r["labels"].items()}
            first["state"] = {k: v.detach().clone() for k, v in r["model"].state_dict().items()}
    fit.run("static", str(tmp_path), paths["infos"], "one_box_est", split=2, n_epoch=1, batch_size=4, lr=0.002,
            weight_decay=1e-3, on_train_step=rec)
    # the same model init: the run's seeds, no torch draw before the model is built
    ev.fix_seed(fit.SEED)
    torch.cuda.manual_seed(fit.SEED)
    model = static_model.StaticModelOneBoxEst(n_classes=3, n_channel=3).to(DEV)
    model.sampler, model.seed = "numpy", fit.SEED
    criterion = static_model.FrustumPointNetLossOneBoxEst()
    optimizer = torch.optim.Adam(model.parameters(), lr=0.002, weight_decay=1e-3)
    torch.set_rng_state(states[0][0])
    np.random.set_state(states[0][1])
    lab = first["labels"]
    model.train()
    output = model(*first["inputs"])
    losses = criterion(output, lab["mask_label"], lab["center_label"], lab["heading_class_label"],
                       lab["heading_residuals_label"], lab["size_class_label"], lab["size_residual_label"])
    optimizer.zero_grad()
    losses["total_loss"].backward()
    optimizer.step()
    got = model.state_dict()
    assert set(got) == set(first["state"])
    for k, v in got.items():
        assert torch.equal(v, first["state"][k]), k
