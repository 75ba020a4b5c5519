"""Crop extraction on the device (3dal_pytorch_amd/csrc/dal3_crops.hip through crops.extract_crops and crops.CropPlan)
on the planted scenes of tests/crop_cases.py: every fill route, both words of the member mask, the 64-point, chunk,
workgroup, scan-trip and detection-batch seams, non-finite points and boxes, the edges of the cull grid, faces of rotated
boxes, capacities that cut inside a round, and a plan re-run on other points. tests/test_crop_route_model.py shows on
the CPU that each scene reaches what it claims.

How a run is judged (crop_route_model.judge): counts, starts, offsets and indices equal the model's exactly, membership
being the oracle's; every coordinate lies within 5 * 2^-53 * (|p0 x| + |p1 y| + |p2 z| + |p3|) of the exact rational value
of pose[:3] @ [x, y, z, 1] (gamma_4: a four-term double-precision dot product in any order, with or without FMA; derived,
not measured); NaN points give NaN rows; and nothing is written behind min(total, capacity) of sentinel-filled buffers."""
import importlib

import numpy as np
import pytest
import torch

import crop_cases as C
import crop_route_model as M

crops = importlib.import_module("3dal_pytorch_amd.crops")
pytestmark = pytest.mark.gpu

SENTINEL, GUARD = -7.0, 64


def _device_points(sweeps):
    return torch.from_numpy(np.concatenate(sweeps).astype(np.float32).reshape(-1, 3)).cuda()


def _extract(c, sweeps, inside):
    """crops.extract_crops -> the run's outputs as judge() takes them; the per-detection views against the oracle"""
    frames = crops.extract_crops(sweeps, c["dets"], c["poses"], return_index=True)
    assert len(frames) == len(sweeps)
    start = frames[0]["point"].start
    for f, rec in enumerate(frames):
        assert len(rec["point"]) == len(rec["index"]) == c["dets"][f].shape[0] == rec["boxes_lidar"].shape[0]
        assert rec["point"].start is start
        for k, idx in enumerate(rec["index"]):
            assert np.array_equal(idx.cpu().numpy(), np.nonzero(inside[f][:, k])[0]), (f, k)
            assert rec["point"][k].shape == (idx.shape[0], 3)
    total = int(start[-1])
    return {"counts": np.diff(start), "start": start, "offsets": start, "total": total,
            "rows": frames[0]["point"].flat[:total].cpu().numpy(), "flat_index": frames[0]["index"].flat[:total].cpu().numpy()}


def _plan(c, sweeps, capacity, order=None):
    """a CropPlan writing into buffers of capacity + GUARD sentinel rows -> (plan, run() -> outputs as judge() takes them)"""
    plan = crops.CropPlan([s.shape[0] for s in sweeps], c["dets"], c["poses"], order=order, capacity=capacity, return_index=True)
    rows = torch.full((capacity + GUARD, 3), SENTINEL, dtype=torch.float64, device="cuda")
    idx = torch.full((capacity + GUARD,), int(SENTINEL), dtype=torch.int32, device="cuda")
    plan.out, plan.idx = rows[:capacity], idx
    d_pts = _device_points(sweeps)

    def run():
        out, offsets = plan.run(d_pts)
        assert out.data_ptr() == rows.data_ptr() and plan.idx is idx
        return {"counts": plan.counts[:plan.K].cpu().numpy(), "start": plan.start.cpu().numpy(), "offsets": offsets.cpu().numpy(),
                "total": plan.total(), "rows": rows.cpu().numpy(), "flat_index": idx.cpu().numpy()}
    return plan, run


def _untouched_behind(got, written):
    return bool((got["rows"][written:] == SENTINEL).all()) and bool((got["flat_index"][written:] == int(SENTINEL)).all())


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.int64) if np.asarray(a[k]).dtype == np.float64 else np.asarray(a[k]),
                              np.asarray(b[k]).view(np.int64) if np.asarray(b[k]).dtype == np.float64 else np.asarray(b[k]))
               for k in ("counts", "start", "offsets", "rows", "flat_index")) and a["total"] == b["total"]


@pytest.mark.parametrize("name", C.NAMES)
def test_case_through_extract_crops_and_crop_plan(name):
    c, inside = C.get(name), C.truth(name)
    order = c.get("order")
    exp = M.expected(c["sweeps"], inside, c["poses"])
    got = _extract(c, c["sweeps"], inside)
    assert M.judge(got, exp, c["sweeps"], c["poses"]) == []
    for f, i in c["all_member"]:                                  # NaN points: in every detection, as NaN rows
        mine = np.nonzero((exp["src"][:, 0] == f) & (exp["src"][:, 1] == i))[0]
        assert mine.size == c["dets"][f].shape[0] and np.isnan(got["rows"][mine]).all()
    # the planned run (in the case's output order, if it has one) into sentinel-filled buffers, twice
    exp = M.expected(c["sweeps"], inside, c["poses"], order=order, capacity=exp["total"] + 7)
    plan, run = _plan(c, c["sweeps"], exp["capacity"], order)
    first = run()
    assert M.judge(first, exp, c["sweeps"], c["poses"]) == []
    assert _untouched_behind(first, exp["total"])
    if order is None:                                             # the same rows as extract_crops gave, bit for bit
        assert np.array_equal(first["rows"][:exp["total"]].view(np.int64), got["rows"].view(np.int64))
    assert _same_bits(run(), first)


def test_capacity_cuts_inside_rounds_track_major():
    c, inside = C.get("capacity"), C.truth("capacity")
    full = M.expected(c["sweeps"], inside, c["poses"], order=c["order"])
    total = full["total"]
    _, run = _plan(c, c["sweeps"], total + 7, c["order"])
    whole = run()
    # a capacity inside frame 0's unique round (some of its rows in front of the cut, some behind) and one between the
    # first and the second member that a detection has in its ordered round
    uniq = sorted(M.round_rows(full, inside[0], 0, 0).values())
    cut_unique = uniq[len(uniq) // 2]
    assert uniq[0] < cut_unique <= uniq[-1]
    twice = sorted(r for (k, _), r in M.round_rows(full, inside[0], 0, 1).items() if k == 2)
    cut_ordered = twice[1]
    assert len(twice) >= 2 and twice[0] < cut_ordered
    for cap in (1, total - 1, total, total + 7, cut_unique, cut_ordered):
        exp = M.expected(c["sweeps"], inside, c["poses"], order=c["order"], capacity=cap)
        plan, run = _plan(c, c["sweeps"], cap, c["order"])
        got = run()
        assert M.judge(got, exp, c["sweeps"], c["poses"]) == [], cap
        written = min(total, cap)
        assert np.array_equal(got["offsets"], np.minimum(full["offsets"], cap)) and got["total"] == total == plan.total()
        assert np.array_equal(got["rows"][:written].view(np.int64), whole["rows"][:written].view(np.int64)), cap
        assert np.array_equal(got["flat_index"][:written], whole["flat_index"][:written]), cap
        assert _untouched_behind(got, written), cap


def test_plan_rerun_on_other_points_equals_a_fresh_plan():
    """counts, chunk counts or rows left over from points A must not show in the run on points B"""
    c = C.get("reuse")
    a, b = c["sweeps"], c["sweeps_b"]
    in_a, in_b = C.truth("reuse"), [C.inside_of(b[0], c["dets"][0])]
    exp_a, exp_b = M.expected(a, in_a, c["poses"]), M.expected(b, in_b, c["poses"])
    for k in c["emptied"]:
        assert exp_a["counts"][k] > 0 and exp_b["counts"][k] == 0
    assert exp_a["counts"][50] == 0 < exp_b["counts"][50] and a[0].shape == b[0].shape
    cap = max(exp_a["total"], exp_b["total"]) + 7
    _, fresh = _plan(c, b, cap)
    want = fresh()
    plan, _ = _plan(c, a, cap)
    d_a, d_b = _device_points(a), _device_points(b)
    plan.run(d_a)
    assert plan.total() == exp_a["total"]
    plan.out.fill_(SENTINEL)                                      # (rows of A behind B's total are no finding)
    plan.idx.fill_(int(SENTINEL))
    out, offsets = plan.run(d_b)
    got = {"counts": plan.counts[:plan.K].cpu().numpy(), "start": plan.start.cpu().numpy(), "offsets": offsets.cpu().numpy(),
           "total": plan.total(), "rows": out.cpu().numpy(), "flat_index": plan.idx.cpu().numpy()[:cap]}
    assert M.judge(got, M.expected(b, in_b, c["poses"], capacity=cap), b, c["poses"]) == []
    want["rows"], want["flat_index"] = want["rows"][:cap], want["flat_index"][:cap]
    assert _same_bits(got, want)
    # without a capacity the first run sizes the buffer; the second, on B, fits it and is judged the same way
    auto = crops.CropPlan([a[0].shape[0]], c["dets"], c["poses"], return_index=True)
    auto.run(d_a)
    assert auto.capacity >= exp_b["total"]
    out, offsets = auto.run(d_b)
    got = {"counts": auto.counts[:auto.K].cpu().numpy(), "start": auto.start.cpu().numpy(), "offsets": offsets.cpu().numpy(),
           "total": auto.total(), "rows": out.cpu().numpy(), "flat_index": auto.idx.cpu().numpy()}
    assert M.judge(got, M.expected(b, in_b, c["poses"], capacity=auto.capacity), b, c["poses"]) == []
