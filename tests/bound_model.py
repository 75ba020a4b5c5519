"""tests/bound_model.py — what the CPU models of the screened layers share (screen_model, head_screen_model,
dec_prune_model; emu16 and dec_sparse_model take the fold only): the oracle's BatchNorm fold in fp32, and the error-bound
coefficients of a layer screened on the fp16 MFMA over K input channels, as the packer evaluates them (csrc/dal3_misc.hip,
bound_coefficients; every model keeps its own K):

  |fp16-MFMA score(c) - fp32 chain(c)| <= X * P_c + Q_c   for a point with ||x||_2 <= X,
  P_c = kappa(K) ||w_c||_2 + 2^-24 sqrt(K),  Q_c = 2^-24 ||w_c||_1 + 2^-40,  kappa(K) = 1.02 * 2^-10 + K * 2^-23,

in float64 with the packer's relative margin of 1e-6.
"""
import numpy as np

from oracle import ref_heads as R


def fold(sd, p, layer, bn):
    w, b = R.fold_bn(sd, p, layer, bn)
    return w.float(), b.float()


def kappa(K):
    return 1.02 * 2.0 ** -10 + K * 2.0 ** -23


def coefficients(w, K):
    w = w.double()
    P = (kappa(K) * w.norm(dim=1) + 2.0 ** -24 * np.sqrt(K)) * (1 + 1e-6)
    Q = (2.0 ** -24 * w.abs().sum(1) + 2.0 ** -40) * (1 + 1e-6)
    return P, Q
