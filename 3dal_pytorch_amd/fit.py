"""File-level training run: `tools/static_train.py` and `tools/dynamic_train.py` of the reference, with the Dataset /
DataLoader replaced by the batched device path of this package and the per-step host metric replaced by one launch —

    trackStatic_{i}.pkl / trackDynamic_{i}.pkl (i < --split) + infos + annos/*.pkl         (SURVEY.md 8(g) formats)
      -> preprocessing + random.shuffle + 10 % validation split        (static_train.py:29-52, dynamic_train.py:30-35)
      -> per epoch: batches in DataLoader(shuffle=True) order          torch's own sampler on the global torch stream
           crops + labels on the device                                prep.prepare_*_batch(..., labels)
           model.train(), forward, criterion, zero_grad, backward, Adam.step
           metrics.TrainMetrics.update                                 one launch, no read-back
         scheduler.step(), eval_one_epoch on the validation split, the reference's log lines and checkpoints

Same command line as the reference's scripts (static_train.py:168-177, dynamic_train.py:135-143):

    python -m 3dal_pytorch_amd.fit static  --track DIR --infos infos.pkl --model_type one_box_est [--split 16] \\
                                           [--n_epoch 100] [--lr 0.001] [--batch_size 64] [--weight_decay 1e-4]
    python -m 3dal_pytorch_amd.fit dynamic --track DIR --infos infos.pkl ...

plus `--sampler numpy|device` (eval.py's meaning) and `--precision fp32|f16x3` (the training kernels' two
arithmetics, train.py). The log goes to <track>/static/log/train/<model_type>.txt or <track>/dynamic/log/train/train.txt,
checkpoints to <track>/static/model/<model_type>/ or <track>/dynamic/model/.

Differences from the reference, all deliberate:
  * the IoU of the metric lines is iou.py's rotated-box IoU in place of the un-vendored fpointnet geometry (the
    substitution eval.box_metrics makes); loss, seg acc and the counts follow the reference's recipe;
  * the step loop reads nothing back: the metrics accumulate on the device and are read once per epoch and phase
    (the numpy sampler's object-point draw in the forward still needs the per-item point counts on the host);
  * with `--sampler numpy` the global NumPy stream is consumed in the reference's order (a batch's item draws, then
    the forward's object-point draws, the dynamic Dataset's substitution of items without their annotation included:
    here the substitute is trained on, as there); `--sampler device` draws on the GPU, keyed on a running item count,
    and stands the next item of the split that has its annotation in for one that lacks it;
  * a validation split of 0 items logs nan where the reference divides by zero, and a run whose eval accuracy is
    never >= the best so far (nan) logs `Model save to None` and saves no checkpoint.
"""
import argparse
import copy
import logging
import os
import pathlib
import pickle
import random

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import eval as ev
from . import metrics, prep

SEED = 10922081                                     # static_train.py:181
VAL_RATIO = 0.1


def lr_lambda(init_lr, step_size=20, gamma=0.7, eta_min=0.00001):
    """the LambdaLR factor of static_train.py:221-225"""
    def f(epoch):
        g = gamma ** (epoch // step_size)
        return g if init_lr * g > eta_min else 0.01
    return f


def load_tracks(track_dir, head, split):
    """trackStatic_{i}.pkl / trackDynamic_{i}.pkl for i < split, merged in order (later keys win, as dict(a + b))"""
    track = {}
    name = "trackStatic" if head == "static" else "trackDynamic"
    for i in range(split):
        with open(os.path.join(track_dir, f"{name}_{i}.pkl"), "rb") as f:
            track.update(pickle.load(f))
    return track


def split_tracks(track, annos=None, ratio=VAL_RATIO):
    """`preprocessing` of static_train.py:29-52 (annos given: the static filter of eval.preprocessing first) and
    dynamic_train.py:30-35: random.shuffle of the items, the first int(ratio * n) for validation"""
    if annos is not None:
        track = ev.preprocessing(track, annos)
    items = list(track.items())
    random.shuffle(items)
    n_val = int(ratio * len(items))
    return dict(items[n_val:]), dict(items[:n_val])


class StaticBatches:
    """STATICTRACK(track) batched on the device: batch(indices) -> ((pts, init_box, bbox_gt), labels)"""
    static = True

    def __init__(self, track, annos, n_points=metrics.NUM_POINT_STATIC, sampler="numpy", seed=SEED, device="cuda"):
        self.tracks = list(track.values())
        self.n_points, self.sampler, self.seed, self.device = n_points, sampler, seed, device
        best = [t["token"][int(np.argmax(np.stack(t["score"])))] for t in self.tracks]
        self.poses = [annos.pose(tok) for tok in best]
        self.gt = [annos.gt_box(tok, t["match"][-1]) for tok, t in zip(best, self.tracks)]

    def __len__(self):
        return len(self.tracks)

    def batch(self, idx, item_offset=0):
        pts, init, lab = prep.prepare_static_batch([self.tracks[k] for k in idx], [self.poses[k] for k in idx],
                                                   n_points=self.n_points, sampler=self.sampler, seed=self.seed,
                                                   item_offset=item_offset, device=self.device,
                                                   gt_boxes=[self.gt[k] for k in idx])
        return (pts, init, lab["bbox_gt"]), lab


class DynamicBatches:
    """DYNAMICTRACK(track) batched on the device: batch(indices) -> ((pts, box, bbox_gt), labels)"""
    static = False

    def __init__(self, track, annos, n_per_frame=metrics.NUM_POINT_DYNAMIC, r=2, s=50, sampler="numpy", seed=SEED,
                 device="cuda"):
        self.tracks = list(track.values())
        self.items = ev._dynamic_items(track, annos)
        self.annos, self.n_per_frame, self.r, self.s = annos, n_per_frame, r, s
        self.sampler, self.seed, self.device = sampler, seed, device
        self.store = prep.TrackStore(self.tracks, device) if self.tracks else None

    def __len__(self):
        return len(self.items)

    def _token(self, t, i):
        return self.tracks[t]["token"][i]

    def _prepare(self, idx, item_offset):
        tr = self.tracks
        return prep.prepare_dynamic_batch(
            self.store, [self.items[k][:2] for k in idx], [self.annos.pose(self._token(*self.items[k][:2])) for k in idx],
            n_per_frame=self.n_per_frame, r=self.r, s=self.s, sampler=self.sampler, seed=self.seed,
            item_offset=item_offset, device=self.device,
            gt_of_frame=lambda t, i: self.annos.gt_box(tr[t]["token"][i], tr[t]["match"][-1]),
            pose_of_frame=lambda t, i: self.annos.pose(tr[t]["token"][i]))

    def batch(self, idx, item_offset=0):
        idx = [int(k) for k in idx]
        if self.sampler == "numpy":
            parts = ev.numpy_stream_parts(idx, self.items, self.tracks, self.r, self.n_per_frame,
                                          lambda seg: self._prepare(seg, 0))
            pts, box, init, lab = ev.join_dynamic_parts(parts)
        else:                                       # the device sampler: every item of a frame without its annotation
            idx = [k if self.items[k][2] else self._substitute(k) for k in idx]
            pts, box, init, lab = self._prepare(idx, item_offset)
        return (pts, box, lab["bbox_gt"]), lab

    def _substitute(self, k):
        """device sampler: the next item (cyclically) that has its annotation, a deterministic stand-in for the
        reference's random pick"""
        n = len(self.items)
        for j in range(1, n + 1):
            if self.items[(k + j) % n][2]:
                return (k + j) % n
        raise ValueError("no item of the split has its matched annotation")


def _as_reference_dtypes(lab):
    """the .float() / .long() the reference's loop applies to the Dataset's tensors (static_train.py:72-81)"""
    out = {k: (v.float() if k in ("bbox_gt", "mask_label", "center_label", "heading_residuals_label",
                                   "size_residual_label") else v.long()) for k, v in lab.items()}
    return out


def _criterion_args(lab):
    return (lab["mask_label"], lab["center_label"], lab["heading_class_label"], lab["heading_residuals_label"],
            lab["size_class_label"], lab["size_residual_label"])


def loader(n, batch_size, shuffle):
    """index batches in the order DataLoader(dataset, batch_size, shuffle) draws them from the global torch stream
    (RandomSampler and the loader's own base-seed draw, torch's code)"""
    return DataLoader(range(n), batch_size=batch_size, shuffle=shuffle)


def train_one_epoch(model, data, criterion, optimizer, batch_size, n_points, two_stage, item_base=0, on_step=None):
    """the train loop of static_train.py:54-92 over one epoch -> (TrainMetrics, items drawn). on_step (tests): called
    after every step with a dict of the step's model, optimizer, indices, inputs, labels, output and loss"""
    m = metrics.TrainMetrics(next(model.parameters()).device, n_points)
    drawn = 0
    for idx in loader(len(data), batch_size, True):
        idx = idx.tolist()
        model.train()
        model.item_offset = item_base + drawn
        inputs, lab = data.batch(idx, item_base + drawn)
        lab = _as_reference_dtypes(lab)
        drawn += len(idx)
        output = model(*inputs)
        losses = criterion(output, *_criterion_args(lab))
        total_loss = losses["total_loss"]
        optimizer.zero_grad()
        total_loss.backward()
        optimizer.step()
        m.update(output, lab, total_loss, two_stage)
        if on_step is not None:
            on_step({"model": model, "optimizer": optimizer, "idx": idx, "inputs": inputs, "labels": lab,
                     "output": output, "loss": total_loss})
    model.item_offset = 0
    return m, drawn


def eval_one_epoch(model, data, criterion, batch_size, n_points, two_stage, on_step=None):
    """eval_one_epoch of static_eval.py:178-211 / dynamic_eval.py:152-211 -> TrainMetrics"""
    m = metrics.TrainMetrics(next(model.parameters()).device, n_points)
    first = 0
    for idx in loader(len(data), batch_size, False):
        idx = idx.tolist()
        model.eval()
        model.item_offset = first
        inputs, lab = data.batch(idx, first)
        lab = _as_reference_dtypes(lab)
        first += len(idx)
        with torch.no_grad():
            output = model(*inputs)
            total_loss = criterion(output, *_criterion_args(lab))["total_loss"]
        m.update(output, lab, total_loss, two_stage)
        if on_step is not None:
            on_step({"model": model, "idx": idx, "inputs": inputs, "labels": lab, "output": output, "loss": total_loss})
    model.item_offset = 0
    return m


def _numbers(m):
    r = m.result()
    return {k: r[k] for k in ("loss", "seg_acc", "iou2d", "iou3d", "iou3d_acc", "n_samples", "n_seg_correct",
                              "n_iou_3d_pass")}


def train(model, train_data, val_data, criterion, optimizer, scheduler, n_epoch, result_dir, logger, batch_size=64,
          n_points=metrics.NUM_POINT_STATIC, static=True, on_train_step=None, on_eval_step=None):
    """`train` of static_train.py:54-165 / dynamic_train.py: returns one dict per epoch {"epoch", "lr", "train",
    "eval", "saved"}, "train" / "eval" = {loss, seg_acc, iou2d, iou3d, iou3d_acc, n_samples, n_seg_correct,
    n_iou_3d_pass}"""
    result_dir = pathlib.Path(result_dir)
    two_stage = getattr(model, "two_stage", False)
    best_state, best_iou3d_acc, savepath = {}, 0.0, None
    history, drawn = [], 0
    for epoch in range(n_epoch):
        lr = optimizer.param_groups[0]["lr"]
        m, n = train_one_epoch(model, train_data, criterion, optimizer, batch_size, n_points, two_stage, drawn,
                               on_train_step)
        drawn += n
        tr = _numbers(m)
        logger.info(f"=== Epoch [{epoch + 1}/{n_epoch}] ===")
        logger.info(f"[Train] loss: {tr['loss']:.4f}, seg acc: {tr['seg_acc']:.4f}")
        logger.info(f"[Train] Box IoU (2D/3D): {tr['iou2d']:.4f}/{tr['iou3d']:.4f}")
        logger.info(f"[Train] Box estimation accuracy (IoU=0.7): {tr['iou3d_acc']:.4f}")
        scheduler.step()
        evr = _numbers(eval_one_epoch(model, val_data, criterion, batch_size, n_points, two_stage, on_eval_step))
        logger.info(f"[Eval] loss: {evr['loss']:.4f}, seg acc: {evr['seg_acc']:.4f}")
        logger.info(f"[Eval] Box IoU (2D/3D): {evr['iou2d']:.4f}/{evr['iou3d']:.4f}")
        logger.info(f"[Eval] Box estimation accuracy (IoU=0.7): {evr['iou3d_acc']:.4f}")
        saved = None
        if evr["iou3d_acc"] >= best_iou3d_acc:
            best_iou3d_acc = evr["iou3d_acc"]
            savepath = result_dir / f"acc{evr['iou3d_acc']:04f}_epoch{epoch + 1:03d}.pth"
            logger.info(f"Model save to {savepath}")
            state = {"epoch": epoch + 1, "train_iou3d_acc": tr["iou3d_acc"], "eval_iou3d_acc": evr["iou3d_acc"],
                     "model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict()}
            torch.save(state, savepath)
            best_state = copy.deepcopy(state)
            saved = savepath
        history.append({"epoch": epoch + 1, "lr": lr, "train": tr, "eval": evr, "saved": saved})
    if static:                                      # static_train.py:163-165 logs the last save before the best one
        logger.info(f"Model save to {savepath}")
    best = result_dir / f"acc{best_iou3d_acc:04f}_best.pth"
    if best_state:
        savepath = best
        torch.save(best_state, best)
    if not static:                                  # dynamic_train.py:129-131
        logger.info(f"Model save to {savepath}")
    logger.info("Done.")
    return history


def _logger(log_file):
    """console + file, as tools/utils.py:31-44; the handlers belong to one run() and are closed by it"""
    logger = logging.getLogger("3dal_pytorch_amd.fit")
    logger.setLevel(logging.INFO)
    logger.propagate = False
    fmt = logging.Formatter("%(asctime)s  %(levelname)5s  %(message)s")
    for h in (logging.StreamHandler(), logging.FileHandler(filename=log_file, mode="w")):
        h.setFormatter(fmt)
        logger.addHandler(h)
    return logger


MODELS = {"one_box_est": ("StaticModelOneBoxEst", "FrustumPointNetLossOneBoxEst"),
          "two_box_est": ("StaticModelTwoBoxEst", "FrustumPointNetLossTwoBoxEst")}


def run(head, track_dir, infos_path, model_type="one_box_est", split=16, n_epoch=100, lr=0.001, batch_size=64,
        weight_decay=1e-4, sampler="numpy", precision="fp32", device="cuda", on_train_step=None, on_eval_step=None):
    """`main()` of static_train.py:167-232 (head='static') / dynamic_train.py:134-185 (head='dynamic'); returns
    train()'s per-epoch history"""
    from . import dynamic_model, static_model
    if head not in ("static", "dynamic"):
        raise ValueError(f"unknown head {head!r}")
    if sampler not in ("numpy", "device"):
        raise ValueError(f"unknown sampler {sampler!r}")
    if precision not in ("fp32", "f16x3"):
        raise ValueError(f"precision {precision!r}: the training kernels run fp32 or f16x3")
    ev.fix_seed(SEED)
    torch.cuda.manual_seed(SEED)
    if head == "static" and model_type not in MODELS:
        raise ValueError(f'No model supports for model type "{model_type}".')
    root = pathlib.Path(track_dir) / head
    result_dir = root / "model" / model_type if head == "static" else root / "model"
    result_dir.mkdir(parents=True, exist_ok=True)
    log_dir = root / "log" / "train"
    log_dir.mkdir(parents=True, exist_ok=True)
    logger = _logger(log_dir / (f"{model_type}.txt" if head == "static" else "train.txt"))
    try:
        logger.info("Load track data")
        track = load_tracks(track_dir, head, split)
        logger.info("Load info data")
        with open(infos_path, "rb") as f:
            infos = ev.reorganize_info(pickle.load(f))
        annos = ev.Annos(infos)
        if head == "static":
            train_track, val_track = split_tracks(track, annos)
            train_data = StaticBatches(train_track, annos, sampler=sampler, device=device)
            val_data = StaticBatches(val_track, annos, sampler=sampler, device=device)
            model_cls, loss_cls = (getattr(static_model, c) for c in MODELS[model_type])
            model = model_cls(n_classes=3, n_channel=3)
            n_points = metrics.NUM_POINT_STATIC
        else:
            train_track, val_track = split_tracks(track)
            train_data = DynamicBatches(train_track, annos, sampler=sampler, device=device)
            val_data = DynamicBatches(val_track, annos, sampler=sampler, device=device)
            model, loss_cls = dynamic_model.DynamicModel(n_classes=3, n_channel=4), dynamic_model.DynamicModelLoss
            n_points = metrics.NUM_POINT_DYNAMIC * metrics.NUM_FRAME
        model = model.to(device)
        model.sampler, model.seed, model.precision = sampler, SEED, precision
        criterion = loss_cls()
        optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
        scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer=optimizer, lr_lambda=lr_lambda(lr))
        logger.info("Start training")
        return train(model, train_data, val_data, criterion, optimizer, scheduler, n_epoch, result_dir, logger,
                     batch_size, n_points, static=(head == "static"), on_train_step=on_train_step,
                     on_eval_step=on_eval_step)
    finally:
        for h in list(logger.handlers):
            logger.removeHandler(h)
            h.close()


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("head", choices=["static", "dynamic"])
    parser.add_argument("--track", required=True, help="Directory of trackStatic_{i}.pkl / trackDynamic_{i}.pkl.")
    parser.add_argument("--infos", required=True, help="Path to infos file.")
    parser.add_argument("--model_type", default="one_box_est", help="Type of model (static head).")
    parser.add_argument("--split", type=int, default=16, help="Number of train split.")
    parser.add_argument("--n_epoch", type=int, default=100, help="Epoch to run.")
    parser.add_argument("--lr", type=float, default=0.001, help="Initial learning rate.")
    parser.add_argument("--batch_size", type=int, default=64, help="Batch Size during training.")
    parser.add_argument("--weight_decay", type=float, default=1e-4, help="Weight Decay of Adam.")
    parser.add_argument("--sampler", choices=["numpy", "device"], default="numpy")
    parser.add_argument("--precision", choices=["fp32", "f16x3"], default="fp32",
                        help="arithmetic of the training kernels (fp32 = the reference's).")
    args = parser.parse_args(argv)
    run(args.head, args.track, args.infos, args.model_type, args.split, args.n_epoch, args.lr, args.batch_size,
        args.weight_decay, args.sampler, args.precision)


if __name__ == "__main__":
    main()
