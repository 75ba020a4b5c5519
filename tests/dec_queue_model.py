"""tests/dec_queue_model.py — a CPU MODEL of the row queue of the fp32 throughput decoder's compacted body
(csrc/dal3_pointmlp.hip, DESIGN.md "Compacted dconv2 - dconv4"; test infrastructure in the style of tests/dec_sparse_model.py).

dconv3 (256 -> 128) and dconv4 (128 -> 128) read a complete post-ReLU input. The dense kernel (mlp_layer_ring) adds, per
output and point, the K terms w_k x_k to an accumulator that starts at the folded bias, one fp32 fmaf after the other in
the CHAIN ORDER

    k-tile kt = 0..K/32-1  >  accumulator register r = 0..15  >  lane half h = 0, 1     (channel 32 kt + tile_chan(r, h))

two terms per MFMA k-step. The compacted body, per wave tile of 32 points:
  1. writes row k = 32 kt + 2 r + h of the queue for every chain index and keeps one live bit per row in mask words
     (live: the row's bits are not all +0);
  2. turns the mask into the list of live chain indices, 64 indices per pass: lane L owns index 64 j + L, its place is the
     count of live rows in the passes before plus the count of live lanes below it, dead lanes write nothing; the
     entries behind the list's end name the row of zeros, whose weights read as zeros;
  3. runs ceil(live / 2) k-steps: step s multiplies list entries 2 s (low half) and 2 s + 1 (high half).
`queue_chain` restates these three steps literally, so that a mistake in the place arithmetic, the order or the pad is
found without a GPU.

dconv2 (512 -> 256) is consumed while dconv1 still produces it, in chunks of 32 channels. `grouped_chain` is its chain when
the compact loop runs once per GROUP of chunks with the odd leftover carried to the next group: group = 1 is the shipped
kernel (tests/dec_sparse_model.py's compact_chain), larger groups are the order a grouped consumer has to keep.

fmaf is dec_sparse_model's: float32(float64(w) * float64(x) + float64(acc)), shared term for term by all chains.
"""
import numpy as np

from dec_sparse_model import TILE, fmaf, tile_chan

ZERO_ROW = 256                                             # DEC_Q_ZERO
LIST_OVER = 32                                             # DEC_Q_OVER: entries behind the list's end


def chain(K):
    """chain index k -> input channel, for a layer of K input channels"""
    return np.array([32 * kt + tile_chan(r, h) for kt in range(K // 32) for r in range(16) for h in (0, 1)])


def dense_chain(w, b, act):
    """w (O,K), b (O,), act (K,P) fp32 -> the dense accumulators (O,P) before the ReLU"""
    K = w.shape[1]
    ch = chain(K)
    acc = np.repeat(b[:, None], act.shape[1], axis=1).astype(np.float32)
    for k in range(K):
        acc = fmaf(w[:, ch[k]][:, None], act[ch[k]][None, :], acc)
    return acc


def live_rows(act):
    """act (K,P) -> bool (P/TILE, K) in chain order: some point of the tile has bits other than +0 (NaN, Inf, -0 are live)"""
    K = act.shape[0]
    a = np.ascontiguousarray(act[chain(K)]).view(np.uint32).reshape(K, -1, TILE)
    return (a != 0).any(axis=2).T


def live_list(mask):
    """bool (K,) in chain order -> the list as the kernel builds it: 64 indices per pass, place = live rows before the
    pass + live lanes below; LIST_OVER entries of ZERO_ROW behind the end"""
    K = mask.shape[0]
    out = np.full(K + LIST_OVER, -1, np.int64)
    cnt = 0
    for j in range(K // 64):
        word = mask[64 * j:64 * j + 64]
        for lane in range(64):
            below = int(word[:lane].sum())                 # v_mbcnt on the pass's 64-bit mask
            if word[lane]:
                assert out[cnt + below] == -1, "two lanes on one place"
                out[cnt + below] = 64 * j + lane
        cnt += int(word.sum())
    out[cnt:cnt + LIST_OVER] = ZERO_ROW
    return out, cnt


def queue_chain(w, b, act):
    """the compacted body's chain for a whole layer -> (accumulators (O,P), k-steps per tile, live rows per tile)"""
    K, P = act.shape
    ch = chain(K)
    masks = live_rows(act)
    wq = np.zeros((ZERO_ROW + 1, w.shape[0]), np.float32)   # chain-ordered weight copy; past its end a load returns zeros
    wq[:K] = w[:, ch].T
    acc = np.repeat(b[:, None], P, axis=1).astype(np.float32)
    steps_all, live_all = [], []
    for t in range(P // TILE):
        sl = slice(t * TILE, (t + 1) * TILE)
        rows = np.zeros((ZERO_ROW + 1, TILE), np.float32)
        rows[:K] = act[ch, sl]
        lst, cnt = live_list(masks[t])
        steps = (cnt + 1) // 2
        a = acc[:, sl]
        for s in range(steps):
            for k in (lst[2 * s], lst[2 * s + 1]):         # low half before high half
                a = fmaf(wq[k][:, None], rows[k][None, :], a)
        acc[:, sl] = a
        steps_all.append(steps)
        live_all.append(cnt)
    return acc, np.array(steps_all), np.array(live_all)


def grouped_chain(w, b, act, group):
    """dconv2's chain with one compact loop per `group` chunks of 32 chain indices: the live rows of the group behind the
    leftover of the groups before, paired two by two; an odd one is carried; the very last one gets a zero partner
    -> (accumulators (O,P), k-steps per tile incl. the padded one)"""
    K, P = act.shape
    ch = chain(K)
    masks = live_rows(act)
    acc = np.repeat(b[:, None], P, axis=1).astype(np.float32)
    steps_all = []
    for t in range(P // TILE):
        sl = slice(t * TILE, (t + 1) * TILE)
        a = acc[:, sl]
        pend, steps = [], 0
        for g0 in range(0, K, 32 * group):
            seq = pend + [k for k in range(g0, g0 + 32 * group) if masks[t, k]]
            for s in range(len(seq) // 2):
                for k in (seq[2 * s], seq[2 * s + 1]):
                    a = fmaf(w[:, ch[k]][:, None], act[ch[k], sl][None, :], a)
                steps += 1
            pend = seq[-1:] if len(seq) % 2 else []
        if pend:
            a = fmaf(w[:, ch[pend[0]]][:, None], act[ch[pend[0]], sl][None, :], a)
            a = fmaf(w[:, ch[pend[0]]][:, None], np.zeros((1, TILE), np.float32), a)
            steps += 1
        acc[:, sl] = a
        steps_all.append(steps)
    return acc, np.array(steps_all)
