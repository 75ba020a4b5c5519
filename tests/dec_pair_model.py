"""tests/dec_pair_model.py — a CPU MODEL of the fp32 decoder's compacted body run by a PAIR of waves on one 32-point tile
(DESIGN.md "Two waves per tile"; test infrastructure beside tests/dec_group_model.py and tests/dec_queue_model.py).

The one-wave kernel keeps its row queue to itself: the LDS operations of one wave execute in order and nothing else needs
saying. Two waves that share the queue need a SCHEDULE: who writes which row into which buffer, where the mask words
meet, who owns the leftover, and where the barriers stand. This file states that schedule as two programs that run
against one shared memory, and judges it twice:

  bits     the accumulators of dconv2, dconv3, dconv4 and the logits are those of `dec_queue_model.grouped_chain`,
           `queue_chain` and the dense dconv5 chain, bit for bit: no output's chain is divided between the waves and every
           chain keeps its terms in the one-wave order.
  hazards  an EPOCH is the stretch between two barriers. Inside an epoch the two waves run in any order, so the memory
           records for every location who wrote and who read it in which epoch and with which meaning (a tag), and notes
           a hazard when a wave reads what the partner writes in the same epoch, writes what the partner reads or writes in
           the same epoch, reads a location nobody wrote, or finds another meaning than it expects. A wave's own accesses
           keep their program order. A schedule without hazards gives the same bits in every interleaving; the runner
           still runs each epoch in both orders of the waves.

The schedule (wave w = 0, 1; G = GROUP chunks per group; a group's rows take 32 G = 128 rows):

  rows      dconv2: chunk j of the plan, at place u = j mod G of group g = j div G, is PRODUCED by wave j mod 2: rows
            128 (g mod 2) + 32 u + 2 r + h — two buffers, rows 0 .. 127 and 128 .. 255, which dconv3 needs only later.
            dconv3: wave w writes the rows of its own four k-tiles, 128 w .. 128 w + 127; dconv4: 64 w .. 64 w + 63.
            Row ZERO_ROW is written once by wave 0 before the first barrier.
  masks     the producer of a chunk publishes its mask word at (g mod 2, u); dconv3's and dconv4's words have places of
            their own, one per k-tile. After the barrier each wave reads all words of the group or layer.
  list      each wave builds the WHOLE list for itself in a list of its own (the place arithmetic is the one-wave kernel's)
            and runs the compact loop over all of it for its half of the out-tiles: dconv2's 4 w .. 4 w + 3 of eight,
            dconv3's and dconv4's 2 w, 2 w + 1 of four.
  leftover  an odd total: EACH wave copies the last entry's row to a leftover row of its own, as the one-wave kernel does,
            and carries the entry in registers. A shared leftover row would be overwritten by the faster wave's next odd
            group while the slower one still reads it as entry 0.
  barriers  one per group, between its production and its consumption: produce(0) | B | consume(0) produce(1) | B |
            consume(1) produce(2) | ... The producer of group g + 2 reaches buffer g mod 2 only after the barrier that both
            waves pass once group g is consumed. Then B | dconv3's rows and words | B | dconv3's loop | B | dconv4's rows
            and words | B | dconv4's loop, dconv5's first half by wave 0 | B | dconv5's second half by wave 1.
  dconv5    ONE chain per logit and lane half, in the one-wave order k-tile 0 .. 3: wave 0 adds its k-tiles 0, 1 starting
            from zero and hands the partial sums over; wave 1 CONTINUES them with k-tiles 2, 3 — it does not add two halves —
            then adds the two lane halves and the bias and stores.

FAULTS names the planted faults that `run_tile(fault=...)` builds; the judge has to reject each.
"""
import numpy as np

from dec_group_model import N_LIST
from dec_queue_model import LIST_OVER, ZERO_ROW, chain, live_list
from dec_sparse_model import TILE, fmaf, tile_chan

GROUP = 4                                                  # DAL3_DEC_GROUP
NULL_K = 512                                               # DEC_NULL_K: the plan's padding channel, zero weights
FAULTS = ("single buffer", "no barrier before dconv3", "leftover of one wave", "dconv5 in two halves")


class Lds:
    """the tile's shared memory with the bookkeeping of the hazard judge (see the module text)"""

    def __init__(self):
        self.val, self.wr, self.rd = {}, {}, {}
        self.epoch = 0
        self.hazards = []

    def write(self, wave, loc, value, tag):
        last = self.wr.get(loc)
        if last is not None and last[0] == self.epoch and last[1] != wave:
            self.hazards.append(("two writers in one epoch", loc, self.epoch))
        if any(e == self.epoch and w != wave for e, w in self.rd.get(loc, ())):
            self.hazards.append(("overwritten before its last reader passed a barrier", loc, self.epoch))
        self.val[loc] = np.array(value, copy=True)
        self.wr[loc] = (self.epoch, wave, tag)
        self.rd[loc] = []

    def read(self, wave, loc, tag):
        last = self.wr.get(loc)
        if last is None:
            self.hazards.append(("read before it is written", loc, self.epoch))
            return np.full(TILE, np.nan, np.float32)
        if last[1] != wave and last[0] == self.epoch:
            self.hazards.append(("read in the epoch the partner writes it", loc, self.epoch))
        if last[2] != tag:
            self.hazards.append(("holds %r, the reader expects %r" % (last[2], tag), loc, self.epoch))
        self.rd[loc].append((self.epoch, wave))
        return self.val[loc]


def _words(rows):
    """rows (n, TILE) fp32 -> bool (n,): the row's bits are not all +0"""
    return (np.ascontiguousarray(rows).view(np.uint32) != 0).any(axis=1)


def _queue_layer(w, lds, name, x_own, K, wq, bias):
    """dconv3 / dconv4 for wave w, between the barrier in front of its rows and the end of its loop (a generator: one
    barrier inside). x_own (K/2, TILE): the wave's half of the post-ReLU input, channels K/2 w .. in channel order.
    -> the wave's accumulators (O/2, TILE) before the ReLU"""
    ch = chain(K)
    half = K // 2
    for k in range(half * w, half * (w + 1)):              # its own k-tiles: row k holds channel ch[k]
        lds.write(w, ("row", k), x_own[ch[k] - half * w], (name, k))
    for kt in range(K // 64 * w, K // 64 * (w + 1)):
        rows = np.stack([x_own[ch[k] - half * w] for k in range(32 * kt, 32 * kt + 32)])
        lds.write(w, ("mask", name, kt), _words(rows), (name, "mask", kt))
    yield
    mask = np.concatenate([lds.read(w, ("mask", name, kt), (name, "mask", kt)) for kt in range(K // 32)])
    lst, cnt = live_list(mask)                             # the wave's own list
    O = wq.shape[1] // 2
    acc = np.repeat(bias[O * w:O * (w + 1), None], TILE, axis=1).astype(np.float32)
    for s in range((cnt + 1) // 2):
        for k in (lst[2 * s], lst[2 * s + 1]):
            x = lds.read(w, ("row", int(k)), "zero" if k == ZERO_ROW else (name, int(k)))
            acc = fmaf(wq[k][O * w:O * (w + 1), None], x[None, :], acc)
    return acc


def _wave(w, lds, act1, pk, nch, W, out, fault):
    """wave w's program; every `yield` is the pair's barrier"""
    G = GROUP
    n_groups = (nch + G - 1) // G
    two_buffers = fault != "single buffer"
    own_pend = fault != "leftover of one wave"
    pend_loc = ("pend", w) if own_pend else ("pend", 0)
    if w == 0:
        lds.write(w, ("row", ZERO_ROW), np.zeros(TILE, np.float32), "zero")

    def produce(g):
        buf = (g % 2) if two_buffers else 0
        for u in range(min(G, nch - G * g)):
            j = G * g + u
            if j % 2 != w:
                continue
            for p in range(32):
                lds.write(w, ("row", 128 * buf + 32 * u + p), act1[32 * j + p], ("d2", j, p))
            lds.write(w, ("mask", "d2", buf, u), _words(act1[32 * j:32 * j + 32]), ("d2", "mask", j))

    # ---- dconv2: out-tiles 4 w .. 4 w + 3
    o2 = slice(128 * w, 128 * w + 128)
    acc = np.repeat(W["b2"][o2, None], TILE, axis=1).astype(np.float32)
    pend, pend_entry, steps2 = 0, (0, ("row", ZERO_ROW), "zero"), 0
    produce(0)
    for g in range(n_groups):
        yield
        buf = (g % 2) if two_buffers else 0
        ng = min(G, nch - G * g)
        words = np.concatenate([lds.read(w, ("mask", "d2", buf, u), ("d2", "mask", G * g + u)) for u in range(ng)])
        lst = [None] * N_LIST                              # the wave's own list: (chain index of the weights, row, tag)
        lst[0] = pend_entry
        total = pend
        for j in range((ng + 1) // 2):                     # 64 list positions per pass, as in dec_group_model.group_list
            word = words[64 * j:64 * j + (64 if 2 * j + 1 < ng else 32)]
            for lane in range(len(word)):
                if word[lane]:
                    place = total + int(word[:lane].sum())
                    assert lst[place] is None or place == 0, "two lanes on one place"
                    pos = 32 * (G * g + 2 * j) + lane
                    lst[place] = (int(pk[pos]), ("row", 128 * buf + 64 * j + lane), ("d2", pos // 32, pos % 32))
            total += int(word.sum())
        for lane in range(LIST_OVER):
            lst[total + lane] = (0, ("row", ZERO_ROW), "zero")
        steps = total // 2
        n_flight = 3                                       # the first steps' rows are read before the leftover's row moves
        early = {e: lds.read(w, lst[e][1], lst[e][2]).copy() for e in range(min(2 * n_flight, 2 * steps))}
        if total % 2:
            k, loc, tag = lst[total - 1]
            if loc != pend_loc:                            # (the old leftover alone: the kernel copies the row onto itself)
                if own_pend or w == 0:
                    lds.write(w, pend_loc, lds.read(w, loc, tag), ("pend",) + tag)
                pend_entry = (k, pend_loc, ("pend",) + tag)
        pend = total % 2
        for s in range(steps):
            for e in (2 * s, 2 * s + 1):
                k, loc, tag = lst[e]
                x = early[e] if e in early else lds.read(w, loc, tag)
                acc = fmaf(W["w2c"][k][o2, None], x[None, :], acc)
        steps2 += steps
        if g + 1 < n_groups:
            produce(g + 1)
    if pend:                                               # the very last live channel: its partner is the row of zeros
        k, loc, tag = pend_entry
        acc = fmaf(W["w2c"][k][o2, None], lds.read(w, loc, tag)[None, :], acc)
        acc = fmaf(W["w2c"][k][o2, None], lds.read(w, ("row", ZERO_ROW), "zero")[None, :], acc)
        steps2 += 1
    out["acc2"][o2] = acc
    out["steps2"][w] = steps2

    # ---- dconv3, dconv4: out-tiles 2 w, 2 w + 1. dconv3's rows overlay both of dconv2's buffers.
    if fault != "no barrier before dconv3":
        yield
    acc = yield from _queue_layer(w, lds, "d3", np.maximum(acc, 0), 256, W["wq3"], W["b3"])
    out["acc3"][64 * w:64 * w + 64] = acc
    yield
    acc = yield from _queue_layer(w, lds, "d4", np.maximum(acc, 0), 128, W["wq4"], W["b4"])
    out["acc4"][64 * w:64 * w + 64] = acc

    # ---- dconv5: per logit o and lane half h one chain over k-tile > q > e, channel 32 kt + 8 q + 4 h + e
    y4 = np.maximum(acc, 0)                                # channels 64 w .. 64 w + 63: k-tiles 2 w, 2 w + 1

    def add(part):
        for kt in (2 * w, 2 * w + 1):
            for q in range(4):
                for e in range(4):
                    for h in (0, 1):
                        c = 32 * kt + tile_chan(4 * q + e, h)
                        for o in (0, 1):
                            part[o, h] = fmaf(W["w5"][o, c], y4[c - 64 * w], part[o, h])
        return part

    zero = np.zeros((2, 2, TILE), np.float32)
    if w == 0:
        part = add(zero)
        for o in (0, 1):
            for h in (0, 1):
                lds.write(w, ("l5", o, h), part[o, h], ("l5", o, h))
        yield
    else:
        yield
        got = np.stack([np.stack([lds.read(w, ("l5", o, h), ("l5", o, h)) for h in (0, 1)]) for o in (0, 1)])
        part = add(zero) + got if fault == "dconv5 in two halves" else add(got.copy())
        out["logits"][:] = (part[:, 0] + part[:, 1]) + W["b5"][:, None]


def run_tile(act1, pk, nch, W, fault=None, order=(0, 1)):
    """act1 (32 nch, TILE): relu(dconv1) of the tile in the plan's list positions; pk: the plan's chain indices (weights of
    dconv2 per list position); W: weights(...). order: which wave runs first inside every epoch.
    -> (out: acc2 (256,T), acc3 (128,T), acc4 (128,T), logits (2,T), steps2 (2,); hazards; barriers)"""
    assert nch % 2 == 0 and 2 <= nch <= 16 and act1.shape == (32 * nch, TILE)
    lds = Lds()
    out = {"acc2": np.zeros((256, TILE), np.float32), "acc3": np.zeros((128, TILE), np.float32),
           "acc4": np.zeros((128, TILE), np.float32), "logits": np.zeros((2, TILE), np.float32), "steps2": [0, 0]}
    progs = [_wave(w, lds, act1, pk, nch, W, out, fault) for w in (0, 1)]
    alive = [True, True]
    while alive[0] and alive[1]:
        for w in order:
            try:
                next(progs[w])
            except StopIteration:
                alive[w] = False
        if alive[0] != alive[1]:
            lds.hazards.append(("the waves do not meet the same barriers", None, lds.epoch))
        lds.epoch += 1
    return out, lds.hazards, lds.epoch - 1


def weights(rng, dead3=None, dead4=None):
    """random folded weights of dconv2 .. dconv5 and the copies the kernel reads. dead3 / dead4: bool (256,) / (128,) in CHAIN
    order — inputs of dconv3 / dconv4 planted dead in every point through a bias no sum of terms gets above"""
    w2 = rng.standard_normal((256, 512)).astype(np.float32)
    w3 = rng.standard_normal((128, 256)).astype(np.float32)
    w4 = rng.standard_normal((128, 128)).astype(np.float32)
    W = {"w2": w2, "w3": w3, "w4": w4, "w5": rng.standard_normal((2, 128)).astype(np.float32),
         "b2": rng.standard_normal(256).astype(np.float32), "b3": rng.standard_normal(128).astype(np.float32),
         "b4": rng.standard_normal(128).astype(np.float32), "b5": rng.standard_normal(2).astype(np.float32)}
    if dead3 is not None:
        W["b2"][chain(256)[dead3]] = np.float32(-1e30)
    if dead4 is not None:
        W["b3"][chain(128)[dead4]] = np.float32(-1e30)
    W["w2c"] = np.zeros((NULL_K + 1, 256), np.float32)     # dw2c: chain order, the null channel last
    W["w2c"][:512] = w2[:, chain(512)].T
    for name, w, K in (("wq3", w3, 256), ("wq4", w4, 128)):  # dw3c / dw4c: past the copy's end a load returns zeros
        W[name] = np.zeros((ZERO_ROW + 1, 128), np.float32)
        W[name][:K] = w[:, chain(K)].T
    return W


def reference_tile(act1, pk, nch, W):
    """the one-wave chains of the same tile from tests/dec_queue_model.py -> (acc2, acc3, acc4, logits, dconv2's k-steps)"""
    import dec_queue_model as Q
    Kp = 32 * GROUP * ((nch + GROUP - 1) // GROUP)         # whole groups: the missing chunks are dead and add no term
    ch = chain(Kp)
    wp, ap = np.zeros((256, Kp), np.float32), np.zeros((Kp, TILE), np.float32)
    wp[:, ch[:32 * nch]] = W["w2c"][np.asarray(pk[:32 * nch])].T
    ap[ch[:32 * nch]] = act1
    acc2, steps2 = Q.grouped_chain(wp, W["b2"], ap, GROUP)
    acc3 = Q.queue_chain(W["w3"], W["b3"], np.maximum(acc2, 0))[0]
    acc4 = Q.queue_chain(W["w4"], W["b4"], np.maximum(acc3, 0))[0]
    y4 = np.maximum(acc4, 0)
    part = np.zeros((2, 2, TILE), np.float32)
    for kt in range(4):
        for q in range(4):
            for e in range(4):
                for h in (0, 1):
                    c = 32 * kt + tile_chan(4 * q + e, h)
                    for o in (0, 1):
                        part[o, h] = fmaf(W["w5"][o, c], y4[c], part[o, h])
    return acc2, acc3, acc4, (part[:, 0] + part[:, 1]) + W["b5"][:, None], int(steps2[0])


def judge(act1, pk, nch, W, fault=None):
    """run the pair in both orders of the waves and hold it to the one-wave chains and to the hazard rules"""
    want = reference_tile(act1, pk, nch, W)
    n_groups = (nch + GROUP - 1) // GROUP
    for order in ((0, 1), (1, 0)):
        out, hazards, barriers = run_tile(act1, pk, nch, W, fault=fault, order=order)
        assert not hazards, hazards[:3]
        assert barriers == n_groups + 5, ("barriers per tile", barriers)
        for name, ref in zip(("acc2", "acc3", "acc4", "logits"), want):
            assert np.array_equal(out[name].view(np.uint32), ref.view(np.uint32)), (name, "differs from the one-wave chain")
        assert out["steps2"] == [want[4], want[4]], "k-steps of dconv2"
    return out
