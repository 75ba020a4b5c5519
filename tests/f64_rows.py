"""The rows of tests/test_gpu_f64_parity.py: the smallest inputs that still take each kernel route, synthesised from seeds
(3dal_pytorch_amd/synth.py), with the float64 truth and the fp32 oracle's yardstick of each (tests/f64_ref.py) computed
once and shared. No GPU: tests/test_f64_ref_cpu.py checks on the CPU that every row's yardstick is usable."""
import functools

import numpy as np
import torch

import f64_ref as F
from _common import dec_min_dead, positions_from_indices, synth
from oracle import ref_heads as R

DEC_MIN_DEAD = dec_min_dead()                              # DAL3_DEC_MIN_DEAD (csrc/dal3_kernels.h)


def with_dconv1_bias(seed, shift):
    """synth weights with `shift` (512,) added to dconv1's folded bias (the BN's beta): tests/test_gpu_dec_sparse.py's recipe"""
    sd = dict(synth.state_dict("static_one", seed=seed))
    sd["ins_seg.dbn1.bias"] = (np.asarray(sd["ins_seg.dbn1.bias"]).astype(np.float32) + shift.astype(np.float32))
    return sd


def odd_live_counts_shift():
    """test_gpu_dec_sparse.test_odd_live_counts_in_every_chunk(extra=0): chunk c keeps 2 c + 1 of its 32 channels alive,
    256 of the 512 entries of the crop's term are negative -> the compacted body"""
    rng = np.random.default_rng(95)
    shift = np.full(512, -1e6)
    for c in range(16):
        shift[32 * c + rng.permutation(32)[:2 * c + 1]] = 1e6
    assert int((shift < 0).sum()) >= DEC_MIN_DEAD
    return shift


# name -> (kind, route, builder of (state dict, inputs as numpy arrays in storage layout), rows judged or None for all)
# route: "latency" (B * tiles <= 512) | "small_job" (throughput family, B * N <= 65536) | "big_job" (above it)
def _static(kind, B, N, seed, sd=None, recentre=False):
    pts, init, gt = synth.static_crops(B, N, seed=seed)
    sd = synth.state_dict(kind, seed=seed) if sd is None else sd
    if recentre:
        lg = R.ins_seg(R.as_torch_sd(sd), torch.from_numpy(pts[:8]).transpose(2, 1))
        sd = synth.recentre_seg_bias(sd, float((lg[:, :, 1] - lg[:, :, 0]).mean()))
    return sd, (pts, init, gt)


def _dynamic(B, seed):
    p, b, i8, _ = synth.dynamic_items(B, seed=seed)
    sd = synth.state_dict("dynamic", seed=seed)
    lg = R.ins_seg(R.as_torch_sd(sd), torch.from_numpy(p[:1, ::8]).transpose(2, 1))
    return synth.recentre_seg_bias(sd, float((lg[:, :, 1] - lg[:, :, 0]).mean())), (p, b, i8)


BIG_ROWS = tuple(range(4)) + tuple(range(7, 92, 11)) + tuple(range(92, 96))     # first 4, 8 at stride 11, last 4
ROWS = {
    "lat_c3_16x256": ("ins_seg", "latency", lambda: _static("static_one", 16, 256, 5), None),
    "lat_c3_5x77": ("ins_seg", "latency", lambda: _static("static_one", 5, 77, 77), None),
    "lat_c3_3x1000": ("ins_seg", "latency", lambda: _static("static_one", 3, 1000, 1000), None),
    "lat_c4_2x5120": ("dynamic", "latency", lambda: _dynamic(2, 6), None),
    "small_job_64x1024": ("static_one", "small_job", lambda: _static("static_one", 64, 1024, 3, recentre=True), None),
    "big_job_96x1024": ("ins_seg", "big_job", lambda: _static("static_one", 96, 1024, 91), BIG_ROWS),
    "dec_compacted_96x1024": ("ins_seg", "big_job",
                              lambda: _static("static_one", 96, 1024, 95, with_dconv1_bias(95, odd_live_counts_shift())),
                              BIG_ROWS),
    "dec_dense_96x1024": ("ins_seg", "big_job",
                          lambda: _static("static_one", 96, 1024, 94, with_dconv1_bias(94, np.full(512, 1e6))), BIG_ROWS),
    "static_two_8x1024": ("static_two", "latency", lambda: _static("static_two", 8, 1024, 12, recentre=True), None),
    "dynamic_4x5120": ("dynamic", "small_job", lambda: _dynamic(4, 8), None),
}
F16X3_ROWS = ("lat_c3_16x256", "big_job_96x1024", "small_job_64x1024")
STANDALONE_ROW = "lat_c3_16x256"


def route_of(B, N):
    """the dispatch of launch_ins_seg_encode / _decode (csrc/dal3_api.hip) by the job's size alone"""
    tiles = B * ((N + 31) // 32)
    return "latency" if tiles <= 512 else ("small_job" if B * N <= 65536 else "big_job")


def _logical(kind, arrays):
    """storage-layout numpy inputs -> the oracle's logical CPU tensors"""
    t = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]
    if kind == "dynamic":
        return (t[0].transpose(2, 1), t[1].transpose(2, 1), t[2])
    return (t[0].transpose(2, 1),) + tuple(t[1:])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: kind, route, sd, arrays (full batch, storage layout), rows (indices judged), forced / choice / mask (the
    fp32 oracle's own mask and draws, teacher-forced into the truth and into the kernels), truth, yardstick (on `rows`)"""
    kind, route, make, rows = ROWS[name]
    sd, arrays = make()
    B, N = arrays[0].shape[:2]
    assert route_of(B, N) == route, (name, route_of(B, N))
    rows = np.arange(B) if rows is None else np.asarray(rows)
    sub = tuple(a[rows] for a in arrays)
    ins = _logical(kind, sub)
    c = {"kind": kind, "route": route, "sd": sd, "arrays": arrays, "rows": rows, "forced": None}
    if kind != "ins_seg":
        assert len(rows) == B, "the full models are judged on every row"
        np.random.seed(4)
        tsd = R.as_torch_sd(sd)
        want = {"static_one": lambda: R.static_one_forward(tsd, ins[0], ins[1]),
                "static_two": lambda: R.static_two_forward(tsd, ins[0], ins[1], ins[2]),
                "dynamic": lambda: R.dynamic_forward(tsd, ins[0], ins[1])}[kind]()
        mask = want["mask"].numpy()
        counts = mask.sum(1)
        idx = want["_indices"]
        c["forced"] = (idx, counts)
        c["mask"] = mask
        c["choice"] = np.stack([positions_from_indices(mask[i], idx[i].numpy()) if counts[i] else
                                np.zeros(idx.shape[1], np.int64) for i in range(B)])
    c["truth"] = F.truth(kind, sd, ins, c["forced"])
    c["yardstick"] = F.yardstick(kind, sd, ins, c["forced"], c["truth"])
    return c
