"""The planted crop scenes (tests/crop_cases.py) hit what they claim, by the model of the kernel's decisions
(tests/crop_route_model.py): a case that silently stops reaching its route or seam fails here, without a GPU. Also: the
model's expected output against the oracle's extract_crops, the soundness of the cull (every oracle member's cell lies in
its detection's rastered rectangle, with geom.cull_spheres as shipped), and the judge itself, which must object to three
plausible faults."""
import importlib

import numpy as np
import pytest

import crop_cases as C
import crop_route_model as M
from _common import synth
from oracle import ref_geom as G

geom = importlib.import_module("3dal_pytorch_amd.geom")


def _rounds(name, f):
    c = C.get(name)
    return M.rounds(c["sweeps"][f], C.truth(name)[f], c["dets"][f].shape[0])


def test_constants_follow_the_source():
    assert M.ROUNDS * 64 == M.CROP_CHUNK and M.CROP_WAVES >= 1 and M.CROP_GRID >= 2 and M.CROP_CELL > 0
    if (M.CROP_GRID, float(M.CROP_CELL)) != (60, 2.5):
        return                                                    # the worked examples below are for the shipped grid
    assert M.cell(np.float32([-1e9, -75.0, -72.5, 0.0, 74.99, 75.0, 1e9, np.nan, np.inf, -np.inf])).tolist() == \
        [0, 0, 1, 30, 59, 59, 59, 0, 59, 0]
    # 3 m around the origin: cells 28 (-5 .. -2.5 m) to 31 (2.5 .. 5 m)
    assert M.raster(np.float32([[0, 0, 0, 9.0], [0, 0, 0, np.inf], [np.nan, 0, 0, 1.0], [500, -500, 0, 4.0]])).tolist() == \
        [[28, 31, 28, 31], [0, 59, 0, 59], [0, 59, 0, 59], [59, 59, 0, 0]]


def test_route_conditions():
    r = lambda d: M.route(np.array([d.get(i, 0) for i in range(64)], np.uint64))
    assert r({}) == "empty" and r({63: 1 << 63}) == "single" and r({0: 5, 9: 5}) == "run"
    assert r({0: 1, 9: 2}) == "unique" and r({0: 1 | 1 << 40, 9: 2}) == "unique"
    assert r({0: 1, 9: 3}) == "ordered" and r({0: 1 << 32, 1: 1, 2: 1 << 32}) == "ordered"


@pytest.mark.parametrize("name", C.NAMES)
def test_case_hits_what_it_claims(name):
    c, inside = C.get(name), C.truth(name)
    for f, chunk, batch, rnd, want in c["routes"]:
        assert M.route(_rounds(name, f)[chunk, batch, rnd]) == want, (f, chunk, batch, rnd)
    for f, i, k in c["members"]:
        assert inside[f][i, k], (f, i, k)
    for f, chunk, batch in c["skips"]:
        m = _rounds(name, f)
        assert not m[chunk, batch].any() and m[chunk].any(), (f, chunk, batch)
    for f, i in c["all_member"]:
        assert inside[f][i].all() and inside[f].shape[1] > 0
    for f, k in c["some"]:
        assert inside[f][:, k].sum() >= 3, (f, k)
    for f, k in c["none"]:
        assert not inside[f][:, k].any(), (f, k)
    for f, (p, d) in enumerate(zip(c["sweeps"], c["dets"])):
        assert p.dtype == np.float32 and d.dtype == np.float32 and inside[f].shape == (p.shape[0], d.shape[0])


def test_route_cases_cover_every_route_and_both_mask_words():
    seen = set()
    for name in C.ROUTE_CASES:
        m = _rounds(name, 0)
        seen |= {M.route(r) for r in m.reshape(-1, 64)}
    assert seen == {"empty", "single", "run", "unique", "ordered"}
    # a detection of batch index >= 32 with a duplicate in the round (s_seen's second word, 32 + ctz(hi))
    m = _rounds("ordered_interleaved", 0)[0, 0, 1]
    assert (m >> np.uint64(50) & np.uint64(1)).sum() == 32 and (m >> np.uint64(7) & np.uint64(1)).sum() == 32
    for a, b in ((3, 40), (31, 32), (62, 63)):
        m = _rounds(f"run_pair_{a}_{b}", 0)[1, 0, 1]
        assert set(int(x) for x in m) == {0, 1 << a | 1 << b}
    assert sorted(bin(int(x)).count("1") for x in _rounds("unique_nested", 0)[0, 0, 0]) == [0, 0] + [1] * 61 + [3]
    for n in (2, 33, 64):
        assert np.count_nonzero(_rounds(f"unique_{n}", 0)[0, 0, 1]) == n
    # carried state: every detection of the four rounds is met by the atomic route and then by the ordered one
    m = _rounds("carried", 0)[1, 0]
    for r in range(4):
        assert {k for k in range(64) if (m[r] >> np.uint64(k) & np.uint64(1)).any()} == ({9, 47} if r == 2 else {2, 9, 33, 47})


def test_seam_cases_sit_on_the_seams():
    sizes = [C.get(f"seam_points_{n}")["sweeps"][0].shape[0] for n in C.SIZES]
    assert sizes == C.SIZES == [s.shape[0] for s in C.get("seam_ragged")["sweeps"]]
    w = M.CROP_WAVES * M.CROP_CHUNK
    assert {0, 1, 63, 64, 65, M.CROP_CHUNK, w - 1, w, w + 1, w + M.CROP_CHUNK + 1} <= set(sizes)
    for n in C.SIZES:                                             # both sides of every chunk boundary, first, last, lane 63
        got = {i for _, i, _ in C.get(f"seam_points_{n}")["members"]}
        want = {0, n - 1, 63} | {c * M.CROP_CHUNK - d for c in range(1, M.n_chunks(n) + 1) for d in (0, 1)}
        assert got == {i for i in want if 0 <= i < n}
    zero = C.SIZES.index(0)
    assert C.get("seam_ragged")["dets"][zero].shape[0] == 3 and C.truth("seam_ragged")[zero].shape == (0, 3)
    c = C.get("seam_scan")
    assert M.n_chunks(c["sweeps"][0].shape[0]) == 65
    assert {i // M.CROP_CHUNK for f, i, _ in c["members"] if f == 0} >= {62, 63, 64}
    assert [d.shape[0] for d in C.get("det_ragged")["dets"]] == C.DET_COUNTS == [0, 1, 63, 64, 65, 127, 128, 129]
    for k in C.DET_COUNTS:
        dets = {d for _, _, d in C.get(f"det_count_{k}")["members"]}
        last = (k - 1) // 64 * 64 if k else 0
        assert dets == {b + j for b in (0, last) for j in (0, 31, 32, 63) if b + j < k}


def test_non_finite_cases_by_the_oracle():
    """a NaN coordinate fails no `>= 0`: such a point is in every detection. An infinite x is +inf on one face of every
    box whose faces are not parallel to the x axis: the oracle puts it in none, and the device must do the same."""
    for k in (65, 129):
        c, inside = C.get(f"nonfinite_points_{k}"), C.truth(f"nonfinite_points_{k}")[0]
        pts = c["sweeps"][0]
        assert np.isnan(pts[0, 0]) and np.isfinite(pts[0, 1:]).all() and np.isnan(pts[70, 2]) and np.isfinite(pts[70, :2]).all()
        assert pts[100, 0] == np.inf and pts[101, 0] == -np.inf and np.isnan(pts[199]).all()
        assert inside[[0, 70, 199]].all() and not inside[[100, 101]].any()
    c, inside = C.get("nonfinite_boxes"), C.truth("nonfinite_boxes")[0]
    assert np.isnan(c["dets"][0][2, 0]) and np.isinf(c["dets"][0][4, 4])
    assert inside[:, 2].all()                                     # a NaN face equation excludes nothing


def test_faces_case_has_both_outcomes_next_to_every_box():
    inside = C.truth("faces")[0]
    assert inside.shape[0] == 3 * 6 * 2 * 5 * 4
    for k in range(3):
        mine = inside[k * 240:(k + 1) * 240, k]
        assert 20 < mine.sum() < 220, mine.sum()
    assert not np.isclose(np.mod(C.get("faces")["dets"][0][:, 8], np.pi / 2), 0.0, atol=0.05).any()


@pytest.mark.parametrize("name", C.NAMES)
def test_cull_soundness(name):
    """every oracle member with finite coordinates falls into a cell that its detection's ball marks"""
    c = C.get(name)
    n_checked = 0
    for pts, box9, inside in zip(c["sweeps"], c["dets"], C.truth(name)):
        rect = M.raster(geom.cull_spheres(G.waymo_boxes(box9)))
        cx, cy = M.cell(pts[:, 0]), M.cell(pts[:, 1])
        i, k = np.nonzero(inside & np.isfinite(pts).all(1)[:, None])
        ok = (rect[k, 0] <= cx[i]) & (cx[i] <= rect[k, 1]) & (rect[k, 2] <= cy[i]) & (cy[i] <= rect[k, 3])
        assert ok.all(), (name, i[~ok][:5], k[~ok][:5])
        n_checked += i.size
    assert n_checked > 0 or name in ("seam_points_0", "det_count_0")


def test_cull_cases_reach_the_grid_edges():
    c = C.get("cull_borders")
    rect = M.raster(geom.cull_spheres(G.waymo_boxes(c["dets"][0])))
    assert rect[3, 1] == M.CROP_GRID - 1 and rect[4, 0] == 0 and rect[5, 2] == 0        # straddlers reach the border cells
    assert rect[6].tolist() == [M.CROP_GRID - 1] * 4                                     # beyond: clamped into the corner cell
    assert (rect[7, 1] - rect[7, 0]) >= 8                                                # the 20 m box spans many cells
    pts = c["sweeps"][0]
    on = np.mod(pts[:, :2], M.CROP_CELL) == 0
    assert on[:, 0].sum() >= 9 and on[:, 1].sum() >= 9                                   # coordinates exactly on cell borders
    whole = M.raster(geom.cull_spheres(G.waymo_boxes(C.get("cull_whole_grid")["dets"][0])))
    assert whole[0].tolist() == [0, M.CROP_GRID - 1, 0, M.CROP_GRID - 1]
    far = C.get("cull_far")
    assert np.abs(far["sweeps"][0][:, :2]).min() > 9.9e3


@pytest.mark.parametrize("seed", [1, 2])
def test_expected_agrees_with_the_oracle_extract_crops(seed):
    pts, box9, _, _, pose = synth.sweep(90 + seed, "rm", n_points=700 * seed, n_boxes=4 + seed)
    inside = C.inside_of(pts, box9)
    exp = M.expected(pts, inside, pose)
    _, _, want = G.extract_crops(pts, box9, pose)
    assert exp["total"] == sum(w.shape[0] for w in want) > 30
    for k, w in enumerate(want):
        lo = exp["start"][k]
        assert exp["counts"][k] == w.shape[0] and np.array_equal(exp["offsets"][k:k + 2], [lo, lo + w.shape[0]])
        assert np.allclose(exp["rows"][lo:lo + w.shape[0]], w, rtol=0, atol=1e-9)
    # the model's own rows (NumPy's float64 product) lie within the judge's derived bound
    assert M.judge({**exp, "flat_index": exp["flat_index"]}, exp, pts, pose) == []


@pytest.mark.parametrize("name", C.NAMES)
def test_expected_and_judge_on_every_case(name):
    """the model's own output (NumPy's float64 rows) passes the judge on every case, capped and in the case's order too"""
    c, inside = C.get(name), C.truth(name)
    exp = M.expected(c["sweeps"], inside, c["poses"])
    assert M.judge(exp, exp, c["sweeps"], c["poses"]) == []
    assert exp["total"] == sum(int(i.sum()) for i in inside) == exp["offsets"][-1]
    cut = M.expected(c["sweeps"], inside, c["poses"], order=c.get("order"), capacity=exp["total"] // 2 + 1)
    assert M.judge(cut, cut, c["sweeps"], c["poses"]) == [] and cut["rows_written"] == min(exp["total"], exp["total"] // 2 + 1)


def test_expected_order_and_capacity():
    c = C.get("capacity")
    full = M.expected(c["sweeps"], C.truth("capacity"), c["poses"], order=c["order"])
    assert np.array_equal(full["start"][c["order"]], full["offsets"][:-1]) and full["offsets"][-1] == full["total"]
    cut = M.expected(c["sweeps"], C.truth("capacity"), c["poses"], order=c["order"], capacity=full["total"] - 1)
    assert cut["rows_written"] == full["total"] - 1 and cut["total"] == full["total"] and cut["offsets"].max() == full["total"] - 1
    assert np.array_equal(cut["rows"], full["rows"][:-1]) and np.array_equal(cut["start"], full["start"])


def test_the_judge_objects_to_plausible_faults():
    """the device's output stands in as `got`; a deliberately wrong `expected` must not be accepted"""
    c, inside = C.get("carried"), C.truth("carried")
    pts, pose = c["sweeps"][0], c["poses"][0]
    good = M.expected(pts, inside[0], pose)
    assert M.judge(good, good, pts, pose) == []

    def wrong(change):
        exp = M.expected(pts, inside[0], pose)
        change(exp)
        return M.judge(good, exp, pts, pose)

    # rows of one unique round swapped: two detections' members of chunk 1, round 0 trade places
    rows = M.round_rows(good, inside[0], 1, 0)
    a, b = rows[(2, M.CROP_CHUNK + 5)], rows[(33, M.CROP_CHUNK + 20)]

    def swap(exp):
        exp["src"][[a, b]] = exp["src"][[b, a]]
        exp["flat_index"][[a, b]] = exp["flat_index"][[b, a]]
        exp["rows"][[a, b]] = exp["rows"][[b, a]]
    found = wrong(swap)
    assert any(s.startswith("index") for s in found) and any(s.startswith("row") for s in found)

    # the last member of a chunk dropped: detection 33's point at CHUNK - 1
    def drop(exp):
        fewer = inside[0].copy()
        fewer[M.CROP_CHUNK - 1, 33] = False
        exp.update(M.expected(pts, fewer, pose))
    found = wrong(drop)
    assert any(s.startswith("counts") for s in found) and any(s.startswith("total") for s in found)

    # one detection's rows shifted by one
    def shift(exp):
        lo, n = int(exp["start"][9]), int(exp["counts"][9])
        for key in ("src", "flat_index", "rows"):
            exp[key][lo:lo + n] = np.roll(exp[key][lo:lo + n], 1, axis=0)
    found = wrong(shift)
    assert any(s.startswith("index") for s in found) and any(s.startswith("row") for s in found)
    shifted = M.expected(pts, inside[0], pose)                   # (the other way round: a run whose rows are shifted)
    shift(shifted)
    found = M.judge(shifted, good, pts, pose)
    assert any("detection 9" in s for s in found) and any(s.startswith("row") for s in found)

    # and a row that is right in every respect but for 2^-40 relative is outside the bound
    off = dict(good, rows=good["rows"].copy())
    off["rows"][3, 0] *= 1.0 + 2.0 ** -40
    assert any(s.startswith("row 3") for s in M.judge(off, good, pts, pose))
