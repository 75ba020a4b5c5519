"""The detection run at file level (tools/dist_test.py), single process:

    python -m 3dal_pytorch_amd.dist_test CONFIG --work_dir DIR --checkpoint CKPT [--speed_test] [--testset] [--mytrain]
        [--precision fp32|fp16|bf16] [--sparse_precision fp32|fp16|bf16]

CONFIG is a reference config file (config.Config.fromfile). The model is built from `cfg.model` (config.build_detector),
the data set from `cfg.data.val` | `.test` | `.mytrain` (waymo.WaymoDataset), the checkpoint loaded through the reference's
door (config.load_checkpoint). Every batch is merged on the device by waymo.SweepLoader and goes through
`model.detect(points, offsets, metadata, point_offsets_device)`: one host synchronisation a batch, the read-back detect
already has. Written: DIR/prediction.pkl ({token: output}, every tensor on the CPU) and then DIR/det_annos.pkl, the
detection-mode part of `_create_pd_detection` (det3d/datasets/waymo/waymo_common.py:67-129, 205-207).

Deliberate departures:
- no detection_pred.bin: the Waymo protos are not available (a line says that it is skipped);
- WORLD_SIZE > 1 is refused: the run is single-process (no DistributedSampler padding, no pickle all-gather);
- `Total time per frame:` counts batches between a third and two thirds of the FRAMES, as the reference's loop does: it is
  a time per frame with --speed_test (batch size 1), its intended use.
"""
import argparse
import os
import pickle
import sys
import time

import torch

from . import config as config_mod
from . import crops, waymo
from .detect import CenterHeadPost
from .eval import Annos
from .track import det_anno

DATASETS = {"WaymoDataset": waymo.WaymoDataset}


def save_pred(pred, root):
    with open(os.path.join(root, "prediction.pkl"), "wb") as f:
        pickle.dump(pred, f)
    print("Saved prediction.pkl")


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Train a 3D object detector.")
    parser.add_argument("config", help="train config file path")
    parser.add_argument("--work_dir", required=True, help="the dir to save logs and models")
    parser.add_argument("--checkpoint", help="the dir to checkpoint which the model read from")
    parser.add_argument("--txt_result", type=bool, default=False,
                        help="whether to save results to standard KITTI format of txt type")
    parser.add_argument("--gpus", type=int, default=1, help="number of gpus to use (only applicable to non-distributed training)")
    parser.add_argument("--launcher", choices=["none", "pytorch", "slurm", "mpi"], default="none", help="job launcher")
    parser.add_argument("--speed_test", action="store_true")
    parser.add_argument("--local_rank", type=int, default=0)
    parser.add_argument("--testset", action="store_true")
    parser.add_argument("--mytrain", action="store_true")
    # additions: the MFMA operand types the detectors already have as attributes
    parser.add_argument("--precision", choices=["fp32", "fp16", "bf16"], default="fp32", help="the neck's and the head's MFMA operands")
    parser.add_argument("--sparse_precision", choices=["fp32", "fp16", "bf16"], default="fp32",
                        help="the sparse 3-D middle's MFMA operands (VoxelNet)")
    return parser.parse_args(argv)


def build_dataset(cfg):
    args = dict(cfg)
    kind = args.pop("type")
    if kind not in DATASETS:
        raise KeyError(f"dataset type {kind!r} is not built here (known: {sorted(DATASETS)})")
    return DATASETS[kind](**args)


def create_pd_detection(detections, infos, result_path, ratio=0.25):
    """_create_pd_detection(tracking=False) as far as det_annos.pkl: per frame the names, the scores, the boxes back in
    Waymo's convention ([x, y, z, l, w, h, r1 = -r2 - pi / 2], crops.waymo_boxes), frame_id and metadata from the frame's
    annotation file; a result path with `train` in it keeps the first `ratio` of the frames. -> det_annos as written"""
    if "train" in result_path:
        detections_list = list(detections.items())
        detections = dict(detections_list[:int(len(detections_list) * ratio)])
    annos = Annos(infos)
    det_annos = []
    for token, detection in detections.items():
        box3d = detection["box3d_lidar"].detach().cpu().numpy()
        det_annos.append(det_anno(detection["label_preds"].detach().cpu().numpy(), detection["scores"].detach().cpu().numpy(),
                                  crops.waymo_boxes(box3d), annos(token), infos[token]))
    with open(os.path.join(result_path, "det_annos.pkl"), "wb") as f:
        pickle.dump(det_annos, f)
    print("Saved det_annos.pkl")
    print("detection_pred.bin is skipped: the Waymo protos are not available here")
    return det_annos


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else list(argv))
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError(f"WORLD_SIZE = {os.environ['WORLD_SIZE']}: the detection run here is single-process (the "
                                  "DistributedSampler's padding and the pickle all-gather are not built)")
    cfg = config_mod.Config.fromfile(args.config)
    cfg.local_rank = args.local_rank
    cfg.work_dir = args.work_dir
    cfg.gpus = args.gpus
    print("Distributed testing: False")
    if args.testset:
        print("Use Test Set")
        dataset = build_dataset(cfg.data.test)
    elif args.mytrain:
        print("Use Train Set")
        dataset = build_dataset(cfg.data.mytrain)
    else:
        print("Use Val Set")
        dataset = build_dataset(cfg.data.val)
    voxel_generator = dataset.voxel_generator if dataset.voxel_generator is not None else cfg.get("voxel_generator")
    if voxel_generator is None:
        raise ValueError("the config names no voxel generator: neither a Voxelization step in the data set's pipeline nor a "
                         "top-level voxel_generator")
    model = config_mod.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg, voxel_generator=voxel_generator)
    config_mod.load_checkpoint(model, args.checkpoint, map_location="cpu")
    model = model.cuda()
    model.eval()
    model.precision = args.precision
    if args.sparse_precision != "fp32":
        model.sparse_precision = args.sparse_precision
    batch_size = cfg.data.samples_per_gpu if not args.speed_test else 1
    loader = waymo.SweepLoader(dataset, batch_size, torch.device("cuda", torch.cuda.current_device()))
    print(f"work dir: {args.work_dir}")

    detections = {}
    start, end = int(len(dataset) / 3), int(len(dataset) * 2 / 3)
    time_start = time_end = 0
    for i, (points, offsets, offsets_device, metadata) in enumerate(loader):
        if i == start:
            torch.cuda.synchronize()
            time_start = time.time()
        if i == end:
            torch.cuda.synchronize()
            time_end = time.time()
        outputs = model.detect(points, offsets, metadata, offsets_device)
        detections.update(CenterHeadPost.to_prediction(outputs))
    print("\n Total time per frame: ", (time_end - time_start) / (end - start) if end > start else float("nan"))

    os.makedirs(args.work_dir, exist_ok=True)
    save_pred(detections, args.work_dir)
    create_pd_detection(detections, waymo.reorganize_info(dataset._waymo_infos), args.work_dir)
    if args.txt_result:
        assert False, "No longer support kitti"
    return detections


if __name__ == "__main__":
    main()
