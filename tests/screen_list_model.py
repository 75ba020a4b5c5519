"""tests/screen_list_model.py — a CPU restatement of the list building of the screened max-pools (csrc/dal3_screen.h:
scr_push_hit's bit order, ScreenHits::park_block, scr_build_lists), step by step as the wave does it.

A wave sweeps `nblk` blocks of 32 channels with `T` tiles of 32 points. Lane l (0..63) holds channel 32 mt + (l & 31) of
block mt and, per tile, 16 accumulator registers r = the points tile_chan(r, l >> 5). Per block a lane collects one hit
word: the slices push (register r, tile j) in the order s = r T + j, every push shifts the word left, so push s ends at
bit 16 T - 1 - s. The words are parked [block][lane]; per lane the hits of every tile and the non-empty blocks are
counted on the way; after the sweep a prefix scan over the lanes gives each lane the positions of its own entries, and
each lane walks its non-empty blocks (last block first) and its words' bits (lowest first)."""
import numpy as np


def tile_chan(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def hit_words(hits):
    """hits: bool [nblk][64 lanes][T][16 registers] -> uint32 [nblk][64], pushed in the sweep's order"""
    nblk, lanes, T, R = hits.shape
    assert lanes == 64 and R == 16 and 16 * T <= 32
    words = np.zeros((nblk, 64), np.uint32)
    for r in range(16):
        for j in range(T):
            words = (words << np.uint32(1)) | hits[:, :, j, r].astype(np.uint32)
    return words


def tile_mask(T, j):
    m = 0
    for s in range(j, 16 * T, T):
        m |= 1 << (16 * T - 1 - s)
    return m


def build_lists(words, T, cap):
    """words: uint32 [nblk][64] -> (counts [T], overflow, lists: T arrays of entries (channel << 8) | point).
    With overflow nothing is written: the lists come back empty."""
    nblk = words.shape[0]
    assert nblk <= 32
    words = words.astype(np.uint64) & np.uint64((1 << (16 * T)) - 1)
    # park_block: per lane counts and the word of non-empty blocks (block mt at bit nblk - 1 - mt)
    n = np.zeros((T, 64), np.int64)
    nz = np.zeros(64, np.int64)
    for mt in range(nblk):
        for lane in range(64):
            w = int(words[mt, lane])
            for j in range(T):
                n[j, lane] += bin(w & tile_mask(T, j)).count("1")
            nz[lane] = (nz[lane] << 1) | min(w, 1)
    # scr_build_lists: inclusive scan, exclusive positions, totals from the last lane
    incl = np.cumsum(n, axis=1)
    pos = incl - n
    counts = [int(incl[j, 63]) for j in range(T)]
    if any(c > cap for c in counts):
        return counts, True, [np.zeros(0, np.uint32) for _ in range(T)]
    slots = np.full(T * cap, -1, np.int64)
    for lane in range(64):
        h = lane >> 5
        z = int(nz[lane])
        while z:
            t = (z & -z).bit_length() - 1
            z &= z - 1
            mt = nblk - 1 - t
            w = int(words[mt, lane])
            assert w
            while w:
                s = 16 * T - 1 - ((w & -w).bit_length() - 1)
                w &= w - 1
                j, r = s % T, s // T
                at = j * cap + int(pos[j, lane])
                pos[j, lane] += 1
                assert at < (j + 1) * cap and slots[at] < 0, "an entry past the cap or written twice"
                slots[at] = ((32 * mt + (lane & 31)) << 8) | tile_chan(r, h)
    lists = []
    for j in range(T):
        part = slots[j * cap:j * cap + counts[j]]
        assert (part >= 0).all() and (slots[j * cap + counts[j]:(j + 1) * cap] < 0).all(), "a hole in the list or an entry past its end"
        lists.append(part.astype(np.uint32))
    return counts, False, lists


def expected_pairs(hits, j):
    """the set of (channel, point) of tile j whose hit is set, straight from the bool array"""
    out = set()
    for mt, lane, r in zip(*np.nonzero(hits[:, :, j, :])):
        out.add((32 * int(mt) + (int(lane) & 31), tile_chan(int(r), int(lane) >> 5)))
    return out
