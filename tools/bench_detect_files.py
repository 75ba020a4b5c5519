#!/usr/bin/env python3
"""Measure the detection run's input path on a synthetic segment at Waymo size and write profiles/bench_detect_files.json:

    python tools/bench_detect_files.py [--frames 198] [--points 180000] [--rounds 2] [--dir DIR] [--out FILE]

The segment is `--frames` frame files of about `--points` points (tools/bench_sparse.py's seeded lidar rings, raw intensity
and elongation as the frame files hold them) in the converter's pickle format, nsweeps = 2, written once under `--dir`. The
model is VoxelNet on the 41 x 1504 x 1504 grid with seeded weights and num_input_features = 6, as bench_sparse.py builds it.

Two routes over the whole segment, batch size 1, alternating `--rounds` times in one job (the page cache is warm for both
after the files are written; the first pass of each route is a warm-up and is not counted):
  loader     waymo.SweepLoader (pinned staging in a background thread, each file uploaded once, dal3_sweep_merge) ->
             VoxelNet.detect
  reference  the reference's formulation per frame: both files unpickled, NumPy tanh, concatenate, the float64 transform,
             hstack on the host, ONE upload of the merged array -> the same VoxelNet.detect
Recorded per route: frames per second of the run (wall clock around the loop, which ends in a device synchronise), each
round's figure, the median and the spread. Beside them the loader's parts, each alone: reading + unpickling + staging one
file (host clock), uploading one file's planes (device events), the merge kernel (device events, median; one launch on each of
40 copies of its inputs and output in turn, 640 MB, so that nothing is cache-resident) with the bytes it must move over its time
against the 8.0 TB/s HBM figure, and `detect` on a resident merged frame (wall clock around a
synchronised call). The merged frames of both routes are compared on the first frames: elongation and time bit for bit,
xyz and the tanh column to 1 float32 ulp (the host's BLAS sums in its own order, and its tanh is NumPy's float32 one).

No pass mark is set on any number. The cloud is synthetic: its occupancy is not Waymo's."""
import argparse
import importlib
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_sparse  # noqa: E402

waymo = importlib.import_module("3dal_pytorch_amd.waymo")
detector = importlib.import_module("3dal_pytorch_amd.detector")
hip = importlib.import_module("3dal_pytorch_amd._hip")

HBM_TBS = 8.0


def write_segment(root, frames, points):
    """-> info_path; frame f's vehicle moves 0.8 m a frame along x"""
    for sub in ("lidar", "annos"):
        os.makedirs(os.path.join(root, "val", sub), exist_ok=True)
    infos = []
    pose = lambda f: np.array([[1.0, 0, 0, 2000.0 + 0.8 * f], [0, 1.0, 0, -3000.0], [0, 0, 1.0, 10.0], [0, 0, 0, 1.0]])  # noqa: E731
    for f in range(frames):
        name = f"seq_0_frame_{f}.pkl"
        g = np.random.default_rng(1000 + f)
        c = bench_sparse.cloud(points + int(g.integers(-2000, 2000)), 100 + f)
        feature = np.stack([g.uniform(0, 1, c.shape[0]) ** 4 * 30.0, c[:, 4] * 1.5], 1).astype(np.float32)
        path = os.path.join(root, "val", "lidar", name)
        with open(path, "wb") as fh:
            pickle.dump({"scene_name": "bench", "frame_name": f"bench_{f}", "frame_id": f,
                         "lidars": {"points_xyz": np.ascontiguousarray(c[:, :3]), "points_feature": feature}}, fh)
        prev = max(f - 1, 0)
        sweep = {"path": os.path.join(root, "val", "lidar", f"seq_0_frame_{prev}.pkl"), "token": f"seq_0_frame_{prev}.pkl",
                 "transform_matrix": np.linalg.inv(pose(f)) @ pose(prev) if f else None, "time_lag": 0.1 if f else 0}
        infos.append({"path": path, "anno_path": os.path.join(root, "val", "annos", name), "token": name, "timestamp": 0.1 * f,
                      "sweeps": [sweep]})
    info_path = os.path.join(root, "infos_val_02sweeps_filter_zero_gt.pkl")
    with open(info_path, "wb") as fh:
        pickle.dump(infos, fh)
    return info_path


def reference_merge(info):
    """loading.py's Waymo branch restated on the host with its own NumPy calls -> (n, 6) float32"""
    def one(path):
        with open(path, "rb") as fh:
            lidars = pickle.load(fh)["lidars"]
        feature = lidars["points_feature"]
        feature[:, 0] = np.tanh(feature[:, 0])
        return np.concatenate([lidars["points_xyz"], feature], axis=-1)
    points = one(info["path"])
    plist, tlist = [points], [np.zeros((points.shape[0], 1))]
    for sweep in info["sweeps"]:
        ps = one(sweep["path"]).T
        if sweep["transform_matrix"] is not None:
            ps[:3, :] = sweep["transform_matrix"].dot(np.vstack((ps[:3, :], np.ones(ps.shape[1]))))[:3, :]
        plist.append(ps.T)
        tlist.append(sweep["time_lag"] * np.ones((ps.shape[1], 1)))
    points = np.concatenate(plist, axis=0)
    return np.hstack([points, np.concatenate(tlist, axis=0).astype(points.dtype)])


def build_model(dev, caps=None):
    torch.manual_seed(0)
    test_cfg = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0], nms=dict(nms_pre_max_size=4096, nms_post_max_size=500,
                    nms_iou_threshold=0.7), score_threshold=0.1, pc_range=list(bench_sparse.RANGE[:2]), out_size_factor=8,
                    voxel_size=list(bench_sparse.VOXEL[:2]))
    det = detector.VoxelNet(
        reader=dict(type="VoxelFeatureExtractorV3", num_input_features=6),
        backbone=dict(type="SpMiddleResNetFHD", num_input_features=6, ds_factor=8),
        neck=dict(type="RPN", layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[128, 256], us_layer_strides=[1, 2],
                  us_num_filters=[256, 256], num_input_features=256),
        bbox_head=dict(type="CenterHead", in_channels=512, tasks=[dict(num_class=3, class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"])],
                       dataset="waymo", weight=2, code_weights=[1.0] * 8,
                       common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2)}),
        test_cfg=test_cfg, max_points=bench_sparse.MAX_POINTS, max_voxels=400000, voxel_size=bench_sparse.VOXEL, pc_range=bench_sparse.RANGE,
        sparse_capacities=caps)
    return det.to(dev).eval()


def _stats(v):
    return {"rounds": [float(x) for x in v], "median": float(np.median(v)), "spread": float(max(v) - min(v))}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=198)
    p.add_argument("--points", type=int, default=180000)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--dir", default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_detect_files.json"))
    a = p.parse_args()
    dev = torch.device("cuda:0")
    tmp = None
    if a.dir is None:
        tmp = tempfile.TemporaryDirectory()
        a.dir = tmp.name
    t0 = time.perf_counter()
    info_path = write_segment(a.dir, a.frames, a.points)
    write_s = time.perf_counter() - t0
    ds = waymo.WaymoDataset(info_path, a.dir, nsweeps=2)
    n = len(ds)
    det = build_model(dev)

    def loader_pass():
        kept = 0
        torch.cuda.synchronize()
        t = time.perf_counter()
        for points, off, off_dev, meta in waymo.SweepLoader(ds, 1, dev):
            kept += sum(int(o["scores"].numel()) for o in det.detect(points, off, meta, off_dev))
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t), kept

    def reference_pass():
        kept = 0
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(n):
            merged = reference_merge(ds.info(i))
            points = torch.from_numpy(merged).to(dev)
            kept += sum(int(o["scores"].numel()) for o in det.detect(points, [0, merged.shape[0]], [ds.metadata(i)]))
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t), kept

    # both routes merge to the same rows
    for i, (points, off, _, _) in zip(range(3), waymo.SweepLoader(ds, 1, dev)):
        want, got = reference_merge(ds.info(i)), points.cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(got[:, [4, 5]].view(np.uint32), want[:, [4, 5]].view(np.uint32)), i
        # (the host's BLAS sums in an order of its own: a coordinate next to a rounding boundary may fall the other way)
        assert np.all(np.abs(got[:, :3].astype(np.float64) - want[:, :3]) <= np.spacing(np.abs(want[:, :3]))), i
        assert np.abs(got[:, 3].astype(np.float64) - want[:, 3]).max() <= 2.0 ** -23, i
    fps = {"loader": [], "reference": []}
    kept = {}
    for rnd in range(a.rounds + 1):                          # round 0 warms both routes
        for route, fn in (("loader", loader_pass), ("reference", reference_pass)):
            rate, kept[route] = fn()
            if rnd:
                fps[route].append(rate)
            print(f"round {rnd} {route}: {rate:.2f} frames/s, {kept[route]} boxes kept", flush=True)
    # ---- the loader's parts, each alone
    path = ds.info(n // 2)["path"]
    host = []
    for _ in range(10):
        t = time.perf_counter()
        planes = waymo.read_frame(path)
        host.append((time.perf_counter() - t) * 1e3)
    up = []
    for _ in range(12):
        dst = [torch.empty(h.shape, dtype=torch.float32, device=dev) for h in planes]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for d, h in zip(dst, planes):
            d.copy_(h, non_blocking=True)
        e1.record()
        e1.synchronize()
        up.append(e0.elapsed_time(e1))
    other = [t.to(dev) for t in waymo.read_frame(ds.info(n // 2 - 1)["path"])]
    sample = [[(dst[0], dst[1], None, 0.0), (other[0], other[1], ds.info(n // 2)["sweeps"][0]["transform_matrix"], 0.1)]]
    rows = dst[0].shape[0] + other[0].shape[0]
    out = torch.empty((rows, 6), dtype=torch.float32, device=dev)
    off_dev = torch.empty(2, dtype=torch.int64, device=dev)
    waymo.merge_sweeps(sample, 2, out=out, point_offsets_device=off_dev)
    # the kernel alone, as a stream from memory: SETS copies of the frame pair and of the output, each with its own resident
    # table, SETS x 16 MB = 2.5 x the 256 MB last-level cache, so that a launch finds neither its input nor its output
    # there; one launch on every set in turn between two events (a single launch is a few microseconds)
    SETS = 40
    sets = []
    for _ in range(SETS):
        pair = [[(dst[0].clone(), dst[1].clone(), None, 0.0), (other[0].clone(), other[1].clone(), sample[0][1][2], 0.1)]]
        table, _, _ = waymo.segment_table(pair, 2)
        sets.append((pair, torch.from_numpy(table.view(np.uint8).copy()).to(dev), torch.empty_like(out)))

    def merges():
        for _, table_dev, o in sets:
            hip.check(hip.lib().dal3_sweep_merge(hip.ptr(table_dev), 1, 2, rows, hip.ptr(o), hip.ptr(off_dev), 0, hip.stream()))
    merge_ms = bench_sparse.timed(merges, 20, 3)[0] / SETS
    assert torch.equal(sets[-1][2], out)
    moved = rows * (12 + 8 + 24) + 2 * 136 + 16
    det_ms = []
    for i in range(15):
        torch.cuda.synchronize()
        t = time.perf_counter()
        det.detect(out, [0, rows], point_offsets_device=off_dev)
        torch.cuda.synchronize()
        det_ms.append((time.perf_counter() - t) * 1e3)
    res = {"bench": "detect_files", "device": torch.cuda.get_device_name(0), "frames": n, "points_per_frame": a.points, "nsweeps": 2,
           "batch_size": 1, "rounds": a.rounds, "write_segment_s": write_s,
           "frames_per_second": {k: _stats(v) for k, v in fps.items()},
           "loader_over_reference": float(np.median(fps["loader"]) / np.median(fps["reference"])),
           "loader_faster_beyond_spread": bool(min(fps["loader"]) > max(fps["reference"])),
           "boxes_kept": kept,
           "parts_ms": {"read_unpickle_stage_one_file_host": float(np.median(host)), "upload_one_file_events": float(np.median(up[2:])),
                        "merge_kernel_events": merge_ms, "detect_resident_frame_wall": float(np.median(det_ms[5:]))},
           "merge_kernel": {"rows": rows, "bytes_moved": moved, "tb_per_s": moved / (merge_ms * 1e-3) / 1e12,
                            "share_of_hbm_peak": moved / (merge_ms * 1e-3) / 1e12 / HBM_TBS, "hbm_peak_tb_per_s": HBM_TBS,
                            "note": "one launch on each of 40 copies of the inputs and the output in turn (640 MB, beyond the 256 MB last-level "
                                    "cache) between two device events, the tables resident: bytes the kernel must move over its time"},
           "raw_bytes_per_frame_file": int(planes[0].numel() * 4 + planes[1].numel() * 4),
           "sparse_capacities": "the safe bounds (None): the frames differ, and a tightened capacity of one could overflow on another",
           "cloud": "synthetic (seeded lidar rings over flat ground): its occupancy is not Waymo's"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
