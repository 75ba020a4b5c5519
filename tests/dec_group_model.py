"""tests/dec_group_model.py — a CPU MODEL of dconv2's grouped consumer in the fp32 throughput decoder's compacted body
(csrc/dal3_pointmlp.hip, DESIGN.md "Compacted dconv2 - dconv4"; test infrastructure beside tests/dec_queue_model.py).

`dec_queue_model.grouped_chain` says in which ORDER a consumer that runs one compact loop per group of dconv1 chunks has
to add its terms. This file restates what the kernel does to get there, step by step, with the kernel's own rows, list
and leftover, so that a mistake in any of them is found without a GPU:

  rows      chunk u of a group (u = 0 .. group - 1) writes register r, lane half h to queue row 32 u + 2 r + h: chain index
            k of group g lives in row k - 32 group g. Every group writes the SAME rows again. Row ZERO_ROW is zeros, row
            PEND_ROW holds the leftover.
  list      per group, entries of two words (weight byte offset k * 1024, float offset row * 32). Entry 0 is written with
            the leftover of the groups before whether there is one or not; the live chain indices follow from place `pend`
            on, 64 indices per pass (lane L of pass j owns index 32 group g + 64 j + L, its place is the count of live rows
            before the pass plus the live lanes below it; a group of one chunk fills half a pass); LIST_OVER entries naming
            the row of zeros lie behind the end.
  steps     total // 2 k-steps; step s multiplies entries 2 s (low half-wave) and 2 s + 1 (high half-wave).
  leftover  an odd total: the last entry's row is copied to PEND_ROW before the next group's rows are written, and the
            entry, now naming PEND_ROW, becomes the next list's entry 0. It stays there through any number of dead groups.
  the end   a leftover after the last group is multiplied with the row of zeros as its partner, both under ITS weights.

The rows are kept in ONE array that every group overwrites, as in LDS: reading a row of an older group gives the newer
group's values, which is what a wrong leftover scheme would do on the device.
"""
import numpy as np

from dec_queue_model import LIST_OVER, ZERO_ROW, chain, live_rows
from dec_sparse_model import TILE, fmaf

PEND_ROW = ZERO_ROW + 1 + (256 + LIST_OVER) // 32          # DEC_G_PEND: behind dconv3's list
N_ROWS = PEND_ROW + 1
N_LIST = 1 + 256 + LIST_OVER


def live_sets(group):
    """the live sets of both test files: name -> bool (512,) of live CHAIN INDICES, for a consumer of `group` chunks per
    loop. Every set leaves at least 200 chain indices dead."""
    rng = np.random.default_rng(100 + group)
    span, n_groups = 32 * group, 16 // group
    sets = {}
    odd = np.zeros(512, bool)                             # an odd count in every group
    for g in range(n_groups):
        n = 1 + (span // 4) * (g % 4)                      # 1, 33, 65, 97 at four chunks per group
        odd[g * span + rng.permutation(span)[:n]] = True
    sets["odd per group"] = odd
    across = np.zeros(512, bool)                             # the leftover waits through every group in between
    across[3] = across[512 - span + 1] = True
    sets["leftover across dead groups"] = across
    edge = np.zeros(512, bool)                             # the last chain index of a group and the first of the next
    edge[span - 1] = True
    edge[span % 512] = True
    sets["group boundary"] = edge
    for name, k in (("only 0", 0), ("only 511", 511)):
        one = np.zeros(512, bool)
        one[k] = True
        sets[name] = one
    sets["nothing live"] = np.zeros(512, bool)
    full = np.zeros(512, bool)                             # the longest list: one group entirely live (half of it at 8)
    g = n_groups // 2
    full[g * span:g * span + (span if group < 8 else span // 2)] = True
    sets["longest list"] = full
    sets["longest list behind a leftover"] = full | sets["only 0"]
    sets["random 0.45"] = rng.random(512) >= 0.45
    return sets


def group_list(words, g, group, pend_entry, pend):
    """words: the group's mask words (bool (32 group,)) -> (list of (weight offset, row offset) entries, total)"""
    lst = [None] * N_LIST
    lst[0] = pend_entry
    total = pend
    for j in range((group + 1) // 2):
        lanes = 64 if 2 * j + 1 < group else 32
        word = words[64 * j:64 * j + lanes]
        for lane in range(lanes):
            if word[lane]:
                place = total + int(word[:lane].sum())     # v_mbcnt
                assert lst[place] is None or place == 0, "two lanes on one place"
                lst[place] = ((32 * (group * g + 2 * j) + lane) * 1024, (64 * j + lane) * 32)
        total += int(word.sum())
    for lane in range(LIST_OVER):
        lst[total + lane] = (0, ZERO_ROW * 32)
    return lst, total


def kernel_chain(w, b, act, group, n_flight=3):
    """the grouped consumer as the kernel runs it -> (accumulators (O,P) before the ReLU, k-steps per tile incl. the last,
    padded one). n_flight: DAL3_DEC_NB (the loop reads entries 2 n_flight steps ahead; they must exist and name valid rows)"""
    K, P = act.shape
    ch = chain(K)
    masks = live_rows(act)
    wc = np.ascontiguousarray(w[:, ch].T)                  # dw2c: the chain-ordered weight copy, row k = 1024 bytes
    acc = np.repeat(b[:, None], P, axis=1).astype(np.float32)
    steps_all = []
    for t in range(P // TILE):
        sl = slice(t * TILE, (t + 1) * TILE)
        a = acc[:, sl]
        rows = np.full((N_ROWS, TILE), np.nan, np.float32)  # LDS: nothing is known of rows never written
        rows[ZERO_ROW] = 0
        pend, pend_entry, steps_t = 0, (0, ZERO_ROW * 32), 0
        for g in range(K // (32 * group)):
            for u in range(group):                         # the producer: every chain index has its fixed row
                k0 = 32 * (group * g + u)
                rows[32 * u:32 * u + 32] = act[ch[k0:k0 + 32], sl]
            lst, total = group_list(masks[t, 32 * group * g:32 * group * (g + 1)], g, group, pend_entry, pend)
            steps = total // 2
            # the first n_flight steps' rows are read before the leftover's row moves (entry 0 may name PEND_ROW itself)
            early = {e: rows[lst[e][1] // 32].copy() for e in range(2 * n_flight)}
            if total % 2:
                off, row = lst[total - 1]
                rows[PEND_ROW] = rows[row // 32].copy()
                pend_entry = (off, PEND_ROW * 32)
            pend = total % 2
            for s in range(steps + 2 * n_flight):          # read ahead: entries exist and stay inside the queue
                for e in (2 * s, 2 * s + 1):
                    assert lst[e] is not None and 0 <= lst[e][1] // 32 < N_ROWS, (g, s, e)
            for s in range(steps):
                for e in (2 * s, 2 * s + 1):
                    off, row = lst[e]
                    assert off % 1024 == 0 and row % 32 == 0
                    x = early[e] if e in early else rows[row // 32]
                    a = fmaf(wc[off // 1024][:, None], x[None, :], a)
            steps_t += steps
        if pend:
            off, row = pend_entry
            a = fmaf(wc[off // 1024][:, None], rows[row // 32][None, :], a)
            a = fmaf(wc[off // 1024][:, None], rows[ZERO_ROW][None, :], a)
            steps_t += 1
        acc[:, sl] = a
        steps_all.append(steps_t)
    return acc, np.array(steps_all)
