"""tests/dec_sparse_model.py — a CPU MODEL of the compacted dconv2 of the fp32 throughput decoder (csrc/dal3_pointmlp.hip,
DESIGN.md "Compacted dconv2"; test infrastructure, numpy/torch, in the style of tests/screen_model.py).

dconv2 (512 -> 256) reads relu(dconv1). The dense kernel adds, per output and point, the 512 terms w_k x_k to an
accumulator that starts at the folded bias, one fp32 fmaf after the other in the CHAIN ORDER

    chunk c = 0..15  >  accumulator register r = 0..15  >  lane half h = 0, 1     (channel 32 c + tile_chan(r, h))

two terms per MFMA k-step. The compacted kernel drops, per wave tile of 32 points, the channels that are +0 in all 32
points, pairs the survivors two by two in the same order (an odd one waits for the next chunk's first survivor, the very
last one is paired with a zero activation) and runs the same fmaf chain on them. This module restates both chains term by
term so that a mistake in the order — a carry that overtakes a chunk, a pad in the wrong place — is found without a GPU.

An fp32 fmaf is modelled as float32(float64(w) * float64(x) + float64(acc)): the product of two fp32 numbers is exact in
float64; the sum is rounded twice, which both chains share term for term — the model is about the ORDER and about
dropped zero terms, not about the last bit of one fmaf.
"""
import numpy as np
import torch

from bound_model import fold as _fold

TILE = 32                                                  # points per wave tile (DAL3_DEC_T = 1)


def tile_chan(r, h):
    """channel, within a 32-channel tile, of accumulator register r in lane half h (csrc/dal3_device.h)"""
    return (r & 3) + 8 * (r >> 2) + 4 * h


CHAIN = np.array([32 * c + tile_chan(r, h) for c in range(16) for r in range(16) for h in (0, 1)])   # k -> channel


def fmaf(w, x, acc):
    return (w.astype(np.float64) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def dense_chain(w2, b2, act):
    """w2 (O,512), b2 (O,), act (512,P) fp32 -> the dense accumulators (O,P) before the ReLU"""
    acc = np.repeat(b2[:, None], act.shape[1], axis=1).astype(np.float32)
    for k in range(512):
        ch = CHAIN[k]
        acc = fmaf(w2[:, ch][:, None], act[ch][None, :], acc)
    return acc


def live_masks(act):
    """act (512,P), P a multiple of TILE -> bool (P/TILE, 512) in chain order: some point of the tile is not +-0"""
    a = act[CHAIN].reshape(512, -1, TILE)
    return ((a.view(np.uint32) & 0x7FFFFFFF) != 0).any(axis=2).T


def compact_chain(w2, b2, act):
    """the compacted kernel's chain -> (accumulators (O,P), k-steps per tile incl. the padded one, dense chunks per tile)"""
    P = act.shape[1]
    acc = np.repeat(b2[:, None], P, axis=1).astype(np.float32)
    masks = live_masks(act)
    steps_all, dense_all = [], []
    for t in range(P // TILE):
        sl = slice(t * TILE, (t + 1) * TILE)
        a = acc[:, sl]
        pend = None                                        # chain index of the channel waiting for a partner
        steps = dense = 0
        for c in range(16):
            live = [32 * c + p for p in range(32) if masks[t, 32 * c + p]]
            if len(live) == 32 and pend is None:           # the register path: 16 dense k-steps
                dense += 1
            seq = ([pend] if pend is not None else []) + live
            for s in range(len(seq) // 2):
                for k in (seq[2 * s], seq[2 * s + 1]):     # low half before high half
                    a = fmaf(w2[:, CHAIN[k]][:, None], act[CHAIN[k], sl][None, :], a)
                steps += 1
            pend = seq[-1] if len(seq) % 2 else None
        if pend is not None:                               # the very last one: its partner is a zero activation
            a = fmaf(w2[:, CHAIN[pend]][:, None], act[CHAIN[pend], sl][None, :], a)
            a = fmaf(w2[:, CHAIN[pend]][:, None], np.zeros((1, TILE), np.float32), a)
            steps += 1
        acc[:, sl] = a
        steps_all.append(steps)
        dense_all.append(dense)
    return acc, np.array(steps_all), np.array(dense_all)


def decoder_inputs(sd, pts, p="ins_seg"):
    """pts (B,Cin,N) fp32 -> the post-ReLU inputs of dconv2, dconv3, dconv4: (B,512,N), (B,256,N), (B,128,N); BN folded,
    fp32 torch arithmetic"""
    x = pts
    outs = []
    for layer, bn in (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3"), ("conv4", "bn4"), ("conv5", "bn5")):
        w, b = _fold(sd, p, layer, bn)
        x = torch.relu(torch.einsum("oc,bcn->bon", w, x) + b[None, :, None])
        outs.append(x)
    g = outs[4].max(dim=2, keepdim=True)[0].expand(-1, -1, pts.shape[2])
    x = torch.cat([outs[1], g], dim=1)
    res = []
    for layer, bn in (("dconv1", "dbn1"), ("dconv2", "dbn2"), ("dconv3", "dbn3")):
        w, b = _fold(sd, p, layer, bn)
        x = torch.relu(torch.einsum("oc,bcn->bon", w, x) + b[None, :, None])
        res.append(x)
    return res


def dead_fractions(x):
    """x (B,C,N) post-ReLU, N a multiple of TILE -> (elements = 0, (tile, channel) all zero, channel zero over the crop)"""
    z = x == 0
    B, C, N = x.shape
    return (float(z.float().mean()), float(z.reshape(B, C, N // TILE, TILE).all(dim=3).float().mean()),
            float(z.all(dim=2).float().mean()))
