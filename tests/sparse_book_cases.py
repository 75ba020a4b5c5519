"""The cases that take the sparse middle's integer bookkeeping (dal3_sp_sort, dal3_sp_downsample, dal3_sp_table,
dal3_sp_table_transposed of csrc/dal3_spconv.hip) to every key width, chunk seam, window and count the entry points
admit. Pure NumPy: builders that return (idx, B, shape), and beside them what each case claims to hit, restated from the
kernels' own arithmetic so that tests/test_sparse_book_cases_cpu.py can assert the claims without a GPU:

  passes      the radix passes of a level, max(1, ceil(bit_length(B * D * H * W) / 8)): `radix_passes` of csrc/dal3_block.h
              called with the level's `none` key B * D * H * W, as launch_sp_sort and launch_sp_downsample call it;
  candidates  the E = capacity x prod(ceil(k / s)) keys sp_candidates_kernel writes, in its layout and by its t / s - j
              enumeration: what the downsample sorts, and whose sorted runs of equal keys lie across the 256-entry tiles
              and the 4096-entry chunks;
  radix       the least-significant-byte-first ping-pong sort, to say which buffer holds what after each pass.

`faulty_book` plants one wrong reading of the bookkeeping at a time, each of a kind the small grids of
tests/test_gpu_sparse.py cannot see.
"""
import functools
import itertools

import numpy as np

import sparse_ref as S

RADIX_CHUNK, TILE, SCAN_BLOCK = 4096, 256, 1024      # dal3_block.h: RADIX_CHUNK, RADIX_BLOCK (= SP_BLOCK), RADIX_SCAN_BLOCK
MARGIN = 37                                     # sentinel rows behind the count, as tests/test_gpu_sparse.py has them


def levels(shape):
    """the shapes the bookkeeping walks: the input's, then every strided stem's that still fits (sparse_gpu.windows)"""
    out = [tuple(shape)]
    for _, _, kernel, stride, padding in S.STEMS[1:]:
        if any(n + 2 * p < k for n, k, p in zip(out[-1], kernel, padding)):
            break
        out.append(S.out_shape(out[-1], kernel, stride, padding))
    return out


def passes(B, shape):
    """radix_passes(B * D * H * W) of dal3_block.h: keys lie in [0, none], 8 bits a pass"""
    return max(1, -(-int(B * int(np.prod(shape, dtype=np.int64))).bit_length() // 8))


def pass_counts(B, shape):
    """-> (the sort's passes at the input level, [the downsample's passes at every strided level])"""
    lv = levels(shape)
    return passes(B, lv[0]), [passes(B, s) for s in lv[1:]]


def admissible(B, shape):
    """sp_grid_ok of csrc/dal3_api.hip"""
    cells = int(np.prod(shape, dtype=np.int64))
    return 1 <= B <= 65535 and all(1 <= n <= 65536 for n in shape) and cells < 2147483647 and cells < 2147483647 // B


def scrambled(tag, idx):
    idx = np.asarray(idx, np.int32).reshape(-1, 4)
    return idx[np.argsort(S.synth.uniform(S.SEED, f"book/{tag}/order", (idx.shape[0],)), kind="stable")]


# ------------------------------------------------------------------------------------- key widths
WIDTH_GRIDS = {
    "k255": (1, (3, 5, 17)), "k256": (2, (2, 8, 8)), "k65535": (3, (5, 17, 257)), "k65536": (2, (32, 32, 32)),
    "k2p24m1": (3, (15, 91, 4097)), "k2p24": (4, (16, 512, 512)),
    "largest": (2, (466, 1103, 2089)),          # B * cells = 2^31 - 4: the most sp_grid_ok admits at B = 2
    "waymo": (4, (41, 1504, 1504)),
}
WIDTH_KEYS = {"k255": 255, "k256": 256, "k65535": 65535, "k65536": 65536, "k2p24m1": 2 ** 24 - 1, "k2p24": 2 ** 24}
FIRST_REFUSED = (2, (3, 32767, 10923))          # B * cells = 2^31 - 2 < 2^31 - 1, but cells = floor((2^31 - 1) / B)


def byte_pairs(none):
    """per byte of the largest key none - 1: pairs of keys below `none` that differ in exactly that byte"""
    out = []
    for p in range(max(1, -(-(none - 1).bit_length() // 8))):
        unit = 256 ** p                         # <= none - 1
        top = min(255, (none - 1) // unit)      # the byte's largest value below none with the bytes under it 0
        # the shared rest: byte p and every byte above it 0, and low + unit < none, so the pair with byte 1 always exists
        low = int(S.synth.uniform(S.SEED, f"book/pair/{none}/{p}", (1,))[0] * min(unit, none - unit))
        out.append([(low, low + v * unit) for v in sorted({1, max(1, top // 2), top}) if low + v * unit < none])
    return out


def width_case(name):
    """a few hundred sites of a WIDTH_GRIDS grid in scrambled order: key 0, the last cell of the last sample, blobs at
    both of those corners and around seeded centres (neighbours exist at every level), and byte_pairs"""
    B, shape = WIDTH_GRIDS[name]
    D, H, W = shape
    none = B * D * H * W
    keys = {0, none - 1}
    for pairs in byte_pairs(none):
        for a, b in pairs:
            keys.update((a, b))
    ext = np.asarray([D, H, W], np.int64)
    centres = [(0, np.zeros(3, np.int64)), (B - 1, ext - 1)]
    u = S.synth.uniform(S.SEED, f"book/{name}/centres", (3, 4))
    centres += [(int(r[0] * B), (r[1:] * ext).astype(np.int64)) for r in u]
    for j, (b, c) in enumerate(centres):
        pts = c[None, :] + np.round(S.synth.normal(S.SEED, f"book/{name}/blob{j}", (70, 3), 0.0, 1.6)).astype(np.int64)
        pts = np.clip(pts, 0, ext - 1)
        keys.update((((b * D + pts[:, 0]) * H + pts[:, 1]) * W + pts[:, 2]).tolist())
    return scrambled(name, S.unkey(np.asarray(sorted(keys), np.int64), shape)), B, shape


# ------------------------------------------------------------------------------------- lengths
LENGTH_GRIDS = {"p2": (2, (25, 27, 33)), "p3": (2, (57, 69, 77))}       # 2 and 3 passes at the sort and at the first downsample
# capacity -> rows. The sort's E is the capacity; the first downsample's is 8 x the capacity (the k3 s2 window)
SORT_CAPS = {c: c - MARGIN for c in (4095, 4096, 4097, 8193)}
DOWN_CAPS = {511: 511, 512: 512, 513: 513,      # E = 4088, 4096, 4104: one chunk, exactly one, one entry over
             2561: 2561 - MARGIN,               # E = 20488 >= 5 x 4096 + 1: 6 chunks, a (256, 6) histogram table, 2 elements per
                                                # scan thread and a last span that is ragged
             32769: 32769 - MARGIN}             # E = 262152: 1025 head-count tiles, 2 per scan thread
LENGTH_CASES = [(g, c) for g in LENGTH_GRIDS for c in (*SORT_CAPS, *DOWN_CAPS) if (g, c) != ("p2", 32769)]


@functools.lru_cache(maxsize=None)
def _nearest_first(grid):
    """the grid's cells by their (jittered) distance to the nearest of four centres, two in either sample"""
    B, shape = LENGTH_GRIDS[grid]
    cells = S.unkey(np.arange(B * int(np.prod(shape)), dtype=np.int64), shape).astype(np.int64)
    u = S.synth.uniform(S.SEED, f"book/len/{grid}/centres", (4, 3), 0.2, 0.8) * np.asarray(shape)
    score = np.full(cells.shape[0], np.inf)
    for j, c in enumerate(u):
        d = ((cells[:, 1:] - c[None, :]) ** 2).sum(1)
        score = np.minimum(score, np.where(cells[:, 0] == j % B, d, np.inf))
    score = score + S.synth.uniform(S.SEED, f"book/len/{grid}/jitter", (cells.shape[0],), 0.0, 2.0)
    return cells[np.argsort(score, kind="stable")].astype(np.int32)


def length_case(grid, capacity):
    """-> (idx, B, shape, capacity): the rows are compact balls around a few centres of both samples, so that an output
    site has many candidates and the runs of equal candidate keys are long"""
    B, shape = LENGTH_GRIDS[grid]
    rows = {**SORT_CAPS, **DOWN_CAPS}[capacity]
    return scrambled(f"len/{grid}/{capacity}", _nearest_first(grid)[:rows]), B, shape, capacity


def scan_shape(n):
    """block_scan_spans<1024> over n elements -> (elements per thread, threads with a full span, length of a last shorter
    span or 0): the threads behind those have none"""
    per = -(-n // SCAN_BLOCK)
    return per, n // per, n % per


# ------------------------------------------------------------------------------------- windows
WINDOW_GRID, WINDOW_B = (5, 7, 9), 2
TRIPLES = list(itertools.product((1, 2, 3), (1, 2, 3), (0, 1, 2)))      # per-axis (kernel, stride, padding)


def window_admitted(n, k, s, p):
    """sp_window_ok of csrc/dal3_api.hip and sparse.downsample on one axis of n cells"""
    return 1 <= k <= 3 and 1 <= s <= 3 and 0 <= p <= 2 and n + 2 * p >= k and (n + 2 * p - k) // s + 1 >= 1


def window_cases():
    """[(kernel, stride, padding)]: three different per-axis windows at a time, dealt so that a case mixes kernels"""
    deal = [TRIPLES[(13 * i) % len(TRIPLES)] for i in range(len(TRIPLES))]         # 13 and 27 are coprime: a permutation
    out = []
    for c in range(0, len(deal), 3):
        r = (c // 3) % 3                        # and the three go to the axes in a rotating order
        z, y, x = deal[c:c + 3][r:] + deal[c:c + 3][:r]
        assert all(window_admitted(n, *t) for n, t in zip(WINDOW_GRID, (z, y, x)))
        out.append(tuple((z[a], y[a], x[a]) for a in range(3)))
    return out


def window_sites():
    """the grid fully active in sample 0, a scrambled subset of it in sample 1"""
    cells = int(np.prod(WINDOW_GRID))
    full = S.unkey(np.arange(cells, dtype=np.int64), WINDOW_GRID)
    part = np.argsort(S.synth.uniform(S.SEED, "book/window/subset", (cells,)), kind="stable")[:cells // 3]
    return scrambled("window", np.concatenate([full, S.unkey(part + cells, WINDOW_GRID)])), WINDOW_B, WINDOW_GRID


# ------------------------------------------------------------------------------------- counts
def count_case():
    """300 scrambled sites of 2 x (25, 7, 9): every stem fits"""
    B, shape = 2, (25, 7, 9)
    order = np.argsort(S.synth.uniform(S.SEED, "book/count", (B * int(np.prod(shape)),)), kind="stable")[:300]
    return S.unkey(order, shape), B, shape


def live(n, capacity):
    """sp_live of csrc/dal3_spconv.hip"""
    return capacity if n is None else min(max(int(n), 0), capacity)


# ------------------------------------------------------------------------------------- the kernels' steps, restated
def candidates(idx, B, shape, kernel, stride, padding, capacity=None, accept_k=False):
    """sp_candidates_kernel: (capacity * cand) int64 keys, entry i * cand + c the c-th candidate output site of row i, the
    output level's `none` where there is none. accept_k: the planted fault t - o * s <= k"""
    osh = S.out_shape(shape, kernel, stride, padding)
    none = B * int(np.prod(osh))
    i = np.asarray(idx, np.int64).reshape(-1, 4)
    per = [-(-k // s) for k, s in zip(kernel, stride)]
    cand = int(np.prod(per))
    out = np.full(((capacity or i.shape[0]), cand), none, np.int64)
    good = S.keys_of(i, B, shape) >= 0
    for c, j in enumerate(itertools.product(*[range(n) for n in per])):
        t = i[:, 1:] + np.asarray(padding)
        o = t // np.asarray(stride) - np.asarray(j)
        rem = t - o * np.asarray(stride)
        ok = good & np.all((o >= 0) & (o < np.asarray(osh)) & ((rem <= np.asarray(kernel)) if accept_k else (rem < np.asarray(kernel))), 1)
        key = ((i[:, 0] * osh[0] + o[:, 0]) * osh[1] + o[:, 1]) * osh[2] + o[:, 2]
        out[:i.shape[0], c] = np.where(ok, key, none)
    return out.reshape(-1), none


def runs_crossing(sorted_keys, none, every):
    """how many runs of equal keys below `none` hold both entry m * every - 1 and entry m * every for some m"""
    k = np.asarray(sorted_keys)
    at = np.arange(every, k.size, every)
    return int(((k[at] == k[at - 1]) & (k[at] < none)).sum())


def radix(keys, n_passes):
    """radix_sort_pairs: -> [buffer 0, buffer 1] after n_passes stable passes, lowest byte first; pass p reads buffer p & 1
    and writes the other"""
    buf = [np.asarray(keys, np.int64).copy(), np.zeros(len(keys), np.int64)]
    for p in range(n_passes):
        src = buf[p & 1]
        buf[(p & 1) ^ 1] = src[np.argsort((src >> (8 * p)) & 255, kind="stable")]
    return buf


# ------------------------------------------------------------------------------------- planted faults
FAULTS = ("buffer_pick", "accepts_remainder_k", "decode_float32", "decode_wrapped_int32")


def _unkey(key, B, shape, fault):
    D, H, W = shape
    key = np.asarray(key, np.int64)
    if fault == "decode_wrapped_int32":         # the divisors W * H and W * H * D as wrapped 32-bit products
        wrap = lambda v: int(np.asarray(v, np.int64).astype(np.int32))
        hw, dhw = wrap(W * H), wrap(wrap(W * H) * D)
        return np.stack([key // dhw, (key // hw) % D, (key // W) % H, key % W], 1).astype(np.int32)
    if fault == "decode_float32":               # the quotients through fp32, exact below 2^24 only
        q = lambda n: np.floor(key.astype(np.float32) / np.float32(n)).astype(np.int64)
        return np.stack([q(D * H * W), q(H * W) % D, q(W) % H, key - q(W) * W], 1).astype(np.int32)
    return S.unkey(key, shape)


def faulty_book(idx, B, shape, fault=None, capacity=None):
    """the sites of every level as the kernels' steps give them, [(sorted site keys of the input level, then per strided
    level the (n_out, 4) output sites)], with one reading wrong:
      buffer_pick            the sorted pairs taken from key[passes == 1] instead of key[passes & 1]: right for 1, 2 and 4
                             passes, and after 3 the buffer that two passes have sorted by the low 16 bits only;
      accepts_remainder_k    sp_candidates_kernel's rejection `t - o * s >= k` written `> k`;
      decode_float32         sp_emit_kernel's decode with quotients that are exact for keys below 2^24 only;
      decode_wrapped_int32   its 64-bit divisors as wrapped 32-bit products.
    None: no fault, and then the sites are sparse_ref.downsample's (asserted by the CPU test)."""
    def pick(bufs, n):
        return bufs[1 if n == 1 else 0] if fault == "buffer_pick" else bufs[n & 1]

    idx = np.asarray(idx, np.int32).reshape(-1, 4)
    cap = capacity or idx.shape[0]
    none = B * int(np.prod(shape))
    k = S.keys_of(idx, B, shape)
    k = np.concatenate([np.where(k < 0, none, k), np.full(cap - k.size, none, np.int64)])
    out = [pick(radix(k, passes(B, shape)), passes(B, shape))]
    for _, _, kernel, stride, padding in S.STEMS[1:len(levels(shape))]:
        osh = S.out_shape(shape, kernel, stride, padding)
        ck, none = candidates(idx, B, shape, kernel, stride, padding, accept_k=fault == "accepts_remainder_k")
        sk = pick(radix(ck, passes(B, osh)), passes(B, osh))
        head = (sk < none) & np.concatenate([[True], sk[1:] != sk[:-1]])        # sp_head
        idx, shape = _unkey(sk[head], B, osh, fault), osh
        out.append(idx)
    return out
