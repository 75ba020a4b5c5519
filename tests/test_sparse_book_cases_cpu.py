"""What tests/sparse_book_cases.py claims its cases hit, asserted without a GPU: the radix pass count of every level, the
sort lengths on their chunk and scan seams, runs of equal candidate keys across tile and chunk boundaries, every admitted
per-axis window, and that the planted bookkeeping faults show on these cases and not on the small grids of
tests/test_gpu_sparse.py. The restated kernel steps are checked against sparse_ref's rulebook on the way."""
import importlib
import time

import numpy as np
import pytest

import sparse_book_cases as K
import sparse_ref as S
from test_gpu_sparse import BOOK_CASES

sparse = importlib.import_module("3dal_pytorch_amd.sparse")
K3S2 = ((3, 3, 3), (2, 2, 2), (1, 1, 1))


def test_the_pass_count_is_radix_passes():
    # dal3_block.h: bits = 1; while (bits < 32 && (max_key >> bits) != 0) ++bits; return (bits + 7) / 8
    def radix_passes(max_key):
        bits = 1
        while bits < 32 and (max_key >> bits) != 0:
            bits += 1
        return (bits + 7) // 8

    for none in (1, 2, 255, 256, 257, 65535, 65536, 65537, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 2):
        assert K.passes(1, (1, 1, none)) == radix_passes(none), none


# the sort's passes at the input level, the downsample's at every strided level sparse_gpu.windows yields
PASSES = {"k255": (1, [1, 1]), "k256": (2, [1, 1]), "k65535": (2, [2, 2]), "k65536": (3, [2, 2, 1, 1]), "k2p24m1": (3, [3, 3, 2]),
          "k2p24": (4, [3, 3, 2]), "largest": (4, [4, 4, 3, 3]), "waymo": (4, [4, 3, 3, 3])}


def test_key_width_cases_reach_every_pass_count():
    from sparse_gpu import windows
    sort_seen, down_seen = set(), set()
    for name, (B, shape) in K.WIDTH_GRIDS.items():
        assert K.admissible(B, shape), name
        sparse._check_grid(B, shape)
        assert K.levels(shape) == [tuple(shape)] + [w[4] for w in windows(shape)], name
        at_sort, at_down = K.pass_counts(B, shape)
        assert (at_sort, at_down) == PASSES[name], name
        sort_seen.add(at_sort)
        down_seen.update(at_down)
        if name in K.WIDTH_KEYS:
            assert B * int(np.prod(shape)) == K.WIDTH_KEYS[name], name
    assert sort_seen == down_seen == {1, 2, 3, 4}
    assert [K.passes(*K.WIDTH_GRIDS[k]) for k in ("k255", "k256", "k65535", "k65536", "k2p24m1", "k2p24")] == [1, 2, 2, 3, 3, 4]
    B, shape = K.WIDTH_GRIDS["waymo"]
    assert [int(B * np.prod(s, dtype=np.int64)).bit_length() for s in K.levels(shape)] == [29, 26, 23, 20, 19]
    assert K.pass_counts(B, shape) == (4, [4, 3, 3, 3])
    B, shape = K.WIDTH_GRIDS["largest"]
    assert 0.99 * (2 ** 31 - 1) < B * int(np.prod(shape, dtype=np.int64)) < 2 ** 31 - 1
    assert not K.admissible(B, (shape[0], shape[1], shape[2] + 1))          # at this B and these two axes, the last that fits


@pytest.mark.parametrize("name", sorted(K.WIDTH_GRIDS))
def test_key_width_cases_hold_what_they_claim(name):
    idx, B, shape = K.width_case(name)
    none = B * int(np.prod(shape, dtype=np.int64))
    key = S.keys_of(idx, B, shape)
    assert (key >= 0).all() and np.unique(key).size == key.size and 100 <= key.size <= 500
    assert 0 in key and none - 1 in key
    assert (np.diff(key) < 0).any() and (np.diff(key) > 0).any()            # scrambled
    have = set(key.tolist())
    n_bytes = -(-(none - 1).bit_length() // 8)
    for p, pairs in enumerate(K.byte_pairs(none)):
        assert pairs and all(a in have and b in have for a, b in pairs), (name, p)
        for a, b in pairs:
            assert [q for q in range(4) if (a >> 8 * q) & 255 != (b >> 8 * q) & 255] == [p]
    assert len(K.byte_pairs(none)) == n_bytes
    # neighbours exist: a table of nothing but its centre would compare nothing
    t = S.table_sorted(idx, idx, B, shape, shape, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    assert (np.delete(t, 13, 0) >= 0).sum() > key.size
    # the restated steps are the rulebook's
    book = K.faulty_book(idx, B, shape)
    assert np.array_equal(book[0], np.sort(key))
    for sites, lv in zip(book[1:], S.STEMS[1:]):
        want, shape = S.downsample(idx, B, shape, *lv[2:])
        assert np.array_equal(sites, want), (name, lv[0])
        idx = want
    assert len(book) == len(K.levels(K.WIDTH_GRIDS[name][1]))


@pytest.mark.parametrize("grid,capacity", K.LENGTH_CASES)
def test_length_cases_sit_on_their_seams(grid, capacity):
    t0 = time.perf_counter()
    idx, B, shape, cap = K.length_case(grid, capacity)
    rows = idx.shape[0]
    assert np.unique(S.keys_of(idx, B, shape)).size == rows and (S.keys_of(idx, B, shape) >= 0).all()
    at_sort, at_down = K.pass_counts(B, shape)
    assert (at_sort, at_down[0]) == {"p2": (2, 2), "p3": (3, 3)}[grid]
    assert sparse.candidates(*K3S2[:2]) == 8
    E = 8 * cap
    ck, none = K.candidates(idx, B, shape, *K3S2, capacity=cap)
    assert ck.size == E
    sk = np.sort(ck)
    assert np.array_equal(S.unkey(np.unique(sk[sk < none]), S.out_shape(shape, *K3S2)), S.downsample(idx, B, shape, *K3S2)[0])
    if capacity in K.SORT_CAPS:
        assert rows == cap - K.MARGIN and cap in (4095, 4096, 4097, 8193)
        assert -(-cap // K.RADIX_CHUNK) == {4095: 1, 4096: 1, 4097: 2, 8193: 3}[cap]
    elif capacity in (511, 512, 513):
        assert rows == cap and E == {511: 4088, 512: 4096, 513: 4104}[cap]
        assert -(-E // K.RADIX_CHUNK) == (2 if cap == 513 else 1)
    elif capacity == 2561:
        chunks = -(-E // K.RADIX_CHUNK)
        per, full, rest = K.scan_shape(256 * chunks)
        assert E >= 5 * 4096 + 1 and chunks == 6 and per == 2 and full < K.SCAN_BLOCK       # threads without a span behind the full ones
    else:
        tiles = -(-E // K.TILE)
        assert (cap, E, tiles) == (32769, 262152, 1025) and K.scan_shape(tiles) == (2, 512, 1)
        assert K.scan_shape(1024)[0] == 1                                   # the smallest table with two elements a thread
    # runs of equal candidate keys lie across the seams
    valid = int((sk < none).sum())
    assert K.runs_crossing(sk, none, K.TILE) >= 1, (grid, capacity)
    if valid > 2 * K.RADIX_CHUNK:
        assert K.runs_crossing(sk, none, K.RADIX_CHUNK) >= 1, (grid, capacity)
    assert valid / np.unique(sk[sk < none]).size > 4                        # clustered: long runs
    assert time.perf_counter() - t0 < 5.0


def test_some_length_case_crosses_a_chunk_seam_on_either_grid():
    for grid in K.LENGTH_GRIDS:
        hit = []
        for g, c in K.LENGTH_CASES:
            if g == grid:
                idx, B, shape, cap = K.length_case(g, c)
                ck, none = K.candidates(idx, B, shape, *K3S2, capacity=cap)
                if K.runs_crossing(np.sort(ck), none, K.RADIX_CHUNK):
                    hit.append(c)
        assert hit, grid


def test_window_cases_cover_every_admitted_window():
    cases = K.window_cases()
    assert 9 <= len(cases) <= 12
    admitted = {t for t in K.TRIPLES if all(K.window_admitted(n, *t) for n in K.WINDOW_GRID)}
    assert len(admitted) == 27                                              # an extent of 5 or more admits them all
    seen = set()
    for kernel, stride, padding in cases:
        per_axis = list(zip(kernel, stride, padding))
        assert len(set(per_axis)) == 3
        seen.update(per_axis)
        osh = sparse.out_shape(K.WINDOW_GRID, kernel, stride, padding)
        assert all(n >= 1 for n in osh)
        sparse._check_grid(K.WINDOW_B, osh)
    assert seen == admitted
    assert any(k < s for k, s, p in seen) and any(p >= k for k, s, p in seen)
    idx, B, shape = K.window_sites()
    cells = int(np.prod(shape))
    key = S.keys_of(idx, B, shape)
    assert B == 2 and (key < cells).sum() == cells and 0 < (key >= cells).sum() < cells and np.unique(key).size == key.size
    for kernel, stride, padding in cases:                                   # the restated candidates are the rulebook's sites
        ck, none = K.candidates(idx, B, shape, kernel, stride, padding)
        want, osh = S.downsample(idx, B, shape, kernel, stride, padding)
        assert np.array_equal(S.unkey(np.unique(ck[ck < none]), osh), want), (kernel, stride, padding)


def test_count_case():
    idx, B, shape = K.count_case()
    assert len(K.levels(shape)) == 5 and idx.shape[0] == 300
    assert [K.live(n, 337) for n in (None, 0, 342, -3, 300)] == [337, 0, 337, 0, 300]


# ------------------------------------------------------------------------------------- the new cases can fail
def _differs(idx, B, shape, fault):
    capacity = idx.shape[0] + K.MARGIN          # sentinel rows behind the count, as every GPU case has them
    good, bad = K.faulty_book(idx, B, shape, None, capacity), K.faulty_book(idx, B, shape, fault, capacity)
    return any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(good, bad))


def _new_cases():
    for name in K.WIDTH_GRIDS:
        yield f"width/{name}", K.width_case(name)
    for grid, cap in K.LENGTH_CASES:
        if cap != 32769:
            yield f"length/{grid}/{cap}", K.length_case(grid, cap)[:3]


def test_planted_faults_show_on_the_new_cases_only():
    """One fault at a time, planted in the restated steps: the wrong ping-pong buffer, the window's rejection off by one, a
    narrow key decode. The old cases are tests/test_gpu_sparse.py's BOOK_CASES. Two of the faults do not separate the new
    cases from the old as literally written, and the test pins why:
      - `t - o * s > k` already shows on the old cases: with kernel 3 and stride 2 the remainder reaches 3. What only the
        new window cases add is the same fault where k < s or k = 2, s = 3 (asserted below on those windows alone);
      - a wrapped 32-bit W * H * D never wraps on a grid sp_grid_ok admits (D * H * W <= B * D * H * W < 2^31 - 1), so
        that decode is the true one everywhere; decode_float32 stands in for a decode that is exact on narrow keys only."""
    seen = {f: {"old": [n for n, (idx, B, shape) in BOOK_CASES.items() if _differs(idx, B, shape, f)],
                "new": [n for n, (idx, B, shape) in _new_cases() if _differs(idx, B, shape, f)]} for f in K.FAULTS}
    for f in ("buffer_pick", "decode_float32"):
        assert seen[f]["new"] and not seen[f]["old"], (f, seen[f])
    assert {n for n in seen["buffer_pick"]["new"] if n.startswith("width/")} >= {"width/k65536", "width/k2p24m1", "width/waymo"}
    assert "width/waymo" in seen["decode_float32"]["new"] and "width/largest" in seen["decode_float32"]["new"]
    assert not seen["decode_wrapped_int32"]["old"] and not seen["decode_wrapped_int32"]["new"]
    assert seen["accepts_remainder_k"]["new"] and seen["accepts_remainder_k"]["old"]
    # the windows no old case has, where that fault shows: one axis with k < s, or k = 2 under s = 3
    idx, B, shape = K.window_sites()
    shown = set()
    for kernel, stride, padding in K.window_cases():
        if 3 in kernel and 2 in [s for k, s in zip(kernel, stride) if k == 3]:
            continue                            # has a k3 s2 axis: the kind the old cases see
        good, _ = K.candidates(idx, B, shape, kernel, stride, padding)
        bad, _ = K.candidates(idx, B, shape, kernel, stride, padding, accept_k=True)
        if not np.array_equal(np.unique(good), np.unique(bad)):
            shown.update((k, s) for k, s in zip(kernel, stride))
    assert shown & {(1, 2), (1, 3), (2, 3)}
