#!/usr/bin/env python3
"""Generate tests/golden/roi_train.npz from the REAL reference (jacky121298/3DAL_PyTorch): its own `ProposalTargetLayer`
(det3d/models/roi_heads/target_assigner/proposal_target_layer.py), `RoIHeadTemplate.assign_targets`, `get_loss` and its two
layer losses (roi_head_template.py) and `RoIHead.forward(training=True)` (roi_head.py), on the seeded inputs of
tests/roi_train_ref.py.

Run only where the reference checkout exists (DAL3_REFERENCE, as tests/golden/gen_roi.py reads it):
    python tests/golden/gen_roi_train.py

The files are loaded by path behind gen_roi.py's stubs. What this machine lacks is replaced, nothing else:
  boxes_iou3d_gpu            (CUDA-only) by tests/iou_ref.py's float64 oracle, rounded to the run's dtype;
  np.random.permutation(n)   by the stable argsort of key[:n], key = draws[b, :M];
  np.random.rand(R)          by pick = draws[b, M:] (the floor of its float64 product equals the float32 rule: asserted);
  torch.randint(0, n, (k,))  by the sample's next k picks through min(int(pick * n), n - 1), the product a float32 one;
  nn.Dropout                 by a multiplier module holding the injected mask (the Sequential indices stay);
  torch.cat                  drops an empty Python list among its operands: subsample_rois' fg-only branch concatenates
                             `bg_inds = []`, which this torch refuses.
In the .double() run Tensor.float() gives float64 (rotate_points_along_z's matrix, as in gen_roi.py, and the soft labels'
`(fg_mask > 0).float()`, which the reference then fills with float64 overlaps).

What is recorded for code sizes 7 and 9 (cases c7, c9: 48 slots, 16 rows a sample, 12 GT rows, the [32, 32] / [16, 48] head on
the 2 x 6 x 9 x 20 map), each from the fp32 modules and from their .double() copies on the same inputs (stored as the fp32
output plus a float32 difference): targets_dict after assign_targets, get_loss()'s three losses, autograd's gradients of
the loss with respect to rcnn_cls and rcnn_reg and to every head parameter, and the updated running statistics; for case
big (500 slots, 128 rows, 60 GT rows, code 9) the targets alone. tests/roi_train_ref.py's restatement is asserted against
both runs, and so are the conditions under which float32 rounding cannot move a discrete decision. Fixed timestamps: a rerun
reproduces the archive byte for byte."""
import copy
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gen_pillars as G  # noqa: E402
import gen_roi as GR  # noqa: E402
import roi_ref as R  # noqa: E402
import roi_train_ref as T  # noqa: E402

INT_KEYS = ("roi_labels", "reg_valid_mask")
FLOAT_KEYS = ("rois", "roi_scores", "gt_of_rois_src", "gt_iou_of_rois", "rcnn_cls_labels", "gt_of_rois")


class Draws:
    """the injected randomness of one forward: sample b's key and picks, the picks consumed in order"""

    def __init__(self, draws, n_slots):
        self.draws, self.n_slots, self.b, self.at = np.asarray(draws, np.float32), n_slots, -1, 0

    def next_sample(self):
        self.b, self.at = self.b + 1, 0

    def permutation(self, n):
        return np.argsort(self.draws[self.b, :n], kind="stable")

    def rand(self, n):
        pick = self.draws[self.b, self.n_slots:self.n_slots + n]
        return pick.astype(np.float64)

    def randint(self, low=0, high=None, size=None, **kw):
        k = size[0]
        pick = self.draws[self.b, self.n_slots + self.at:self.n_slots + self.at + k]
        assert low == 0 and len(pick) == k
        self.at += k
        return torch.as_tensor(T.draw(pick, high))


class patched:
    def __init__(self, draws, layer):
        self.d, self.layer = draws, layer

    def __enter__(self):
        self.saved = (np.random.permutation, np.random.rand, torch.randint, self.layer.subsample_rois, torch.cat)
        cat = torch.cat
        sub = self.saved[3]

        def subsample(max_overlaps):
            self.d.next_sample()
            n_fg = int((max_overlaps >= min(self.layer.roi_sampler_cfg.REG_FG_THRESH, self.layer.roi_sampler_cfg.CLS_FG_THRESH)).sum())
            if n_fg:                            # the fg-only case's float64 floor is the float32 rule
                pick = self.d.rand(self.layer.roi_sampler_cfg.ROI_PER_IMAGE)
                assert np.array_equal(np.floor(pick * n_fg).astype(np.int64), T.draw(pick.astype(np.float32), n_fg))
            return sub(max_overlaps=max_overlaps)
        np.random.permutation, np.random.rand, torch.randint = self.d.permutation, self.d.rand, self.d.randint
        torch.cat = lambda ts, *a, **k: cat([t for t in ts if not (isinstance(t, list) and not t)], *a, **k)
        self.layer.subsample_rois = subsample

    def __exit__(self, *exc):
        np.random.permutation, np.random.rand, torch.randint, self.layer.subsample_rois, torch.cat = self.saved


class float_as:
    """while it lasts, Tensor.float() converts to `dtype`"""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.orig = orig = torch.Tensor.float
        if self.dtype == torch.float64:
            torch.Tensor.float = lambda t, *a, **k: t.double()

    def __exit__(self, *exc):
        torch.Tensor.float = self.orig


class Mask(nn.Module):
    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask.to(x.dtype).unsqueeze(-1)


def import_reference():
    GR.import_reference()
    G._stub("det3d.ops.iou3d_nms.iou3d_nms_utils", boxes_iou3d_gpu=lambda a, b: T.iou3d(a.detach().numpy(), b.detach().numpy(), a.dtype))
    G._load_file("det3d.models.roi_heads.target_assigner.proposal_target_layer",
                 "det3d/models/roi_heads/target_assigner/proposal_target_layer.py")
    G._load_file("det3d.models.roi_heads.roi_head_template", "det3d/models/roi_heads/roi_head_template.py")
    return G._load_file("det3d.models.roi_heads.roi_head", "det3d/models/roi_heads/roi_head.py")


def all_features(bev, inp, dtype):
    """roi_features (B, M, num_point * C) as reorder_first_stage_pred_and_feature leaves them: zero rows for the empty slots"""
    rois, labels = torch.as_tensor(inp["rois"]).to(dtype), torch.as_tensor(inp["roi_labels"])
    fake = dict(rois=rois, sample=torch.where(labels != 0, 0, -1))
    return T.gather_features(bev, fake, dtype=dtype)


def batch_dict(inp, feats, dtype):
    return dict(rois=torch.as_tensor(inp["rois"]).to(dtype), roi_scores=torch.as_tensor(inp["roi_scores"]).to(dtype),
                roi_labels=torch.as_tensor(inp["roi_labels"]).long(), gt_boxes_and_cls=torch.as_tensor(inp["gt_boxes_and_cls"]).to(dtype),
                roi_features=feats, batch_size=len(inp["rois"]))


def run_reference(head, case, dtype):
    """forward(training=True), get_loss and backward at `dtype` -> roi_train_ref.run's dictionary"""
    head = copy.deepcopy(head).to(dtype).train()
    masks = [torch.as_tensor(m) for m in case["masks"]]
    for seq in (head.shared_fc_layer, head.cls_layers, head.reg_layers):
        for i, m in enumerate(seq):
            if isinstance(m, nn.Dropout):
                seq[i] = Mask(masks.pop(0))
    assert not masks
    inp = case["inp"]
    feats = all_features(case["bev"], inp, dtype)
    with patched(Draws(inp["draws"], inp["rois"].shape[1]), head.proposal_target_layer), float_as(dtype):
        head(batch_dict(inp, feats, dtype), training=True)
        ret = head.forward_ret_dict
        ret["rcnn_cls"].retain_grad()
        ret["rcnn_reg"].retain_grad()
        total, tb = head.get_loss()
        total.backward()
    out = {k: ret[k].detach() for k in INT_KEYS + FLOAT_KEYS}
    out.update(features=ret["roi_features"].detach(), rcnn_cls=ret["rcnn_cls"].detach(), rcnn_reg=ret["rcnn_reg"].detach(),
               loss=torch.stack([tb["rcnn_loss_cls"], tb["rcnn_loss_reg"], total.detach()]), d_cls=ret["rcnn_cls"].grad,
               d_reg=ret["rcnn_reg"].grad, grads={k: p.grad for k, p in head.named_parameters()},
               stats={k: v for k, v in head.state_dict().items() if "running" in k},
               tracked={k: int(v) for k, v in head.state_dict().items() if "num_batches" in k})
    assert abs(tb["rcnn_loss"] - float(total.detach())) == 0
    return out


def targets_reference(head, inp, dtype):
    head = copy.deepcopy(head).to(dtype)
    feats = torch.zeros(inp["rois"].shape[:2] + (1,), dtype=dtype)
    with patched(Draws(inp["draws"], inp["rois"].shape[1]), head.proposal_target_layer), float_as(dtype):
        tg = head.assign_targets(batch_dict(inp, feats, dtype))
    return {k: tg[k].detach() for k in INT_KEYS + FLOAT_KEYS}


def flat(r):
    out = {k: r[k].numpy() for k in FLOAT_KEYS + ("features", "rcnn_cls", "rcnn_reg", "loss", "d_cls", "d_reg") if k in r}
    for group in ("grads", "stats"):
        for k, v in r.get(group, {}).items():
            out[f"{group}/{k}"] = v.numpy()
    return out


def compare_and_store(out, tag, ref32, ref64, mine32, mine64):
    for k in INT_KEYS:
        assert torch.equal(ref32[k], ref64[k]) and torch.equal(ref32[k], mine64[k]) and torch.equal(ref32[k], mine32[k]), (tag, k)
        out[f"{tag}_{k}"] = ref32[k].numpy().astype(np.int64)
    a32, a64, m32, m64 = flat(ref32), flat(ref64), flat(mine32), flat(mine64)
    for name in a64:
        err = np.abs(m64[name] - a64[name]).max() / max(np.abs(a64[name]).max(), 1e-30)
        same = np.array_equal(m32[name], a32[name])
        print(f"{tag} {name:44s} {str(a64[name].shape):14s} restatement f64 err {err:.1e}, f32 bits {'equal' if same else 'differ'}")
        assert err < 1e-10, (tag, name, err)
        if name in ("rois", "roi_scores", "gt_of_rois_src"):
            assert same and np.array_equal(a32[name].astype(np.float64), a64[name]), (tag, name)
        GR.store(out, tag, name.replace("/", "."), a32[name], a64[name])


def check_stability(tag, inp, cfg, r64):
    """float32 rounding cannot move a discrete decision"""
    for b in range(inp["rois"].shape[0]):
        rois, labels = T._t(inp["rois"][b], T.F64), torch.as_tensor(inp["roi_labels"][b]).long()
        gt = T._t(inp["gt_boxes_and_cls"][b], T.F64)
        iou = T.iou3d(rois[:, :7], gt[:, :7], T.F64)
        same = labels[:, None] == gt[:, -1].long()[None, :]
        masked = torch.where(same, iou, torch.zeros_like(iou))
        top = torch.sort(masked, 1, descending=True).values
        best = top[:, 0].numpy()
        second = top[:, 1].numpy() if top.shape[1] > 1 else np.zeros_like(best)
        assert min(float(np.abs(best - t).min()) for t in T.THRESHOLDS) >= 1e-3, (tag, b)
        assert (((best - second) >= 1e-3) | ((best == 0) & (second == 0))).all(), (tag, b)
    rois, src = r64["rois"], r64["gt_of_rois_src"]
    ry = T.limit_period(rois[:, :, 6], 0.5, np.pi * 2)
    h = ((src[:, :, 6] - ry) % (2 * np.pi)).numpy()
    gap = min(float(np.abs(h - v).min()) for v in (np.pi / 2, 3 * np.pi / 2, np.pi))
    assert gap >= 1e-3, (tag, gap)
    if "rcnn_cls" in r64:
        code = rois.shape[-1]
        assert float(r64["rcnn_cls"].abs().max()) < 10
        assert float((r64["rcnn_reg"] - r64["gt_of_rois"][..., :code].reshape(-1, code)).abs().min()) > 1e-4
    print(f"{tag}: heading gap {gap:.2e}")


def main():
    torch.set_num_threads(1)
    hmod = import_reference()
    out = {}
    for code in (7, 9):
        tag, case = f"c{code}", T.golden_case(code)
        cfg = copy.deepcopy(case["cfg"])
        cfg["LOSS_CONFIG"] = dict(cfg["LOSS_CONFIG"], LOSS_WEIGHTS=dict(cfg["LOSS_CONFIG"]["LOSS_WEIGHTS"]))
        cfg["LOSS_CONFIG"]["LOSS_WEIGHTS"]["code_weights"] = cfg["LOSS_CONFIG"]["LOSS_WEIGHTS"]["code_weights"][:code]
        head = hmod.RoIHead(R.NUM_POINT * R.MAP["C"], GR.Cfg(cfg), num_class=1, code_size=code)
        head.load_state_dict({k: torch.as_tensor(v) for k, v in case["sd"].items()}, strict=True)
        ref = {dt: run_reference(head, case, dt) for dt in (torch.float32, torch.float64)}
        mine = {dt: T.run(case["sd"], case["cfg"], case["bev"], case["inp"], case["masks"], dt) for dt in ref}
        assert all(v == 8 for v in ref[torch.float32]["tracked"].values())
        compare_and_store(out, tag, ref[torch.float32], ref[torch.float64], mine[torch.float32], mine[torch.float64])
        assert torch.equal(mine[torch.float64]["slot"], mine[torch.float32]["slot"])
        out[f"{tag}_slot"] = mine[torch.float64]["slot"].numpy().astype(np.int64)
        out[f"{tag}_sample"] = mine[torch.float64]["sample"].numpy().astype(np.int64)
        # the slots are the restatement's: the reference's rows must be the rows of those slots
        assert np.array_equal(case["inp"]["rois"][np.arange(2)[:, None], out[f"{tag}_slot"]], ref[torch.float32]["rois"].numpy())
        check_stability(tag, case["inp"], case["cfg"], mine[torch.float64])
    inp = T.big_inputs()
    cfg = dict(T.CFG, TARGET_CONFIG=dict(T.TARGET, ROI_PER_IMAGE=T.BIG["R"]))
    head = hmod.RoIHead(32, GR.Cfg(cfg), num_class=1, code_size=9)
    ref = {dt: targets_reference(head, inp, dt) for dt in (torch.float32, torch.float64)}
    mine = {dt: T.targets(inp, cfg["TARGET_CONFIG"], dt) for dt in ref}
    compare_and_store(out, "big", ref[torch.float32], ref[torch.float64], mine[torch.float32], mine[torch.float64])
    out["big_slot"] = mine[torch.float64]["slot"].numpy().astype(np.int64)
    out["big_sample"] = mine[torch.float64]["sample"].numpy().astype(np.int64)
    assert np.array_equal(inp["rois"][0][out["big_slot"][0]], ref[torch.float32]["rois"].numpy()[0])
    check_stability("big", inp, cfg, mine[torch.float64])
    path = os.path.join(HERE, "roi_train.npz")
    G.save(path, out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
