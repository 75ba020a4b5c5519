"""tests/pointnet_pack_cases.py — the fixed small networks whose packed blobs tests/golden/pointnet_blobs.npz pins
(tests/test_gpu_pointnet_pack.py; written by tests/golden/gen_pointnet_blobs.py).

Every value comes from numpy's legacy RandomState, whose streams are frozen across numpy versions, seeded per (head,
layer); torch's generator is not used. BatchNorm of the clean cases: gamma of both signs with |gamma| in [0.5, 1.5],
running variance in [0.5, 2], non-zero mean and beta, so |gamma / sqrt(var + eps)| lies in [0.35, 2.2].

A planted case is a clean fp32 case (its TWIN) with one change that must reach one guard of the packers:
  conv5_big        a folded conv5 weight >= 65504                   -> ins_seg scr_flag
  dconv1a_big      a folded dconv1 per-point-column weight >= 65504 -> ins_seg prn_flag
  dconv2_inf       a +Inf dconv2 weight                             -> ins_seg dec_flag
  dconv3_nan       a NaN dconv3 weight                              -> ins_seg dec_flag
  dconv2_negzero   a folded -0 bias of dconv2 (gamma < 0, b = mean, beta = -0: (+0) * s + (-0) = -0) -> dec_flag
  dconv4_negzero   the same in dconv4                               -> dec_flag
  conv4_big        a static box_est conv4 weight >= 65504           -> the head's scr_flag
  x3_overflow      f16x3 ins_seg with a folded conv3 weight beyond fp16's range: packed as NaN. _hip.pack refuses it on the
                   host, so this case goes to dal3_pack_weights directly (pack() below does that for every case).
FLAG_FROM_END gives, for the flag a plant must set, the flag word's distance in floats from the end of the fp32 blob's
sections (the blob's byte count minus the 32-KiB tail): the sections behind it in csrc/dal3_api.hip's walks.
"""
import ctypes as C
import importlib
import zlib

import numpy as np
import torch
from torch import nn

hip = importlib.import_module("3dal_pytorch_amd._hip")
arch = importlib.import_module("3dal_pytorch_amd.arch")

PAGE = 4096
TAIL_BYTES = 8192 * 4                                       # DAL3_BLOB_TAIL_FLOATS
BIG = 1.0e6                                                 # x 0.35 (the smallest |BN scale|) is still > 65504
DTYPES = ("fp32", "bf16", "fp16", "f16x3")


def _table(t):
    return t["convs"] + t["fcs"]


HEADS = {                                                   # name -> (head kind, [(layer, bn, c_in, c_out)], layer is a Linear from)
    "ins_seg3": (hip.HEAD_INS_SEG, arch.ins_seg_layers(3), 10),
    "ins_seg4": (hip.HEAD_INS_SEG, arch.ins_seg_layers(4), 10),
    "static_box_est": (hip.HEAD_STATIC_BOX_EST, _table(arch.STATIC_BOX_EST), 4),
    "point_emb": (hip.HEAD_POINT_EMB, _table(arch.POINT_EMB), 4),
    "box_emb": (hip.HEAD_BOX_EMB, _table(arch.BOX_EMB), 4),
    "dynamic_box_est": (hip.HEAD_DYNAMIC_BOX_EST, _table(arch.DYNAMIC_BOX_EST), 0),
}

# sections behind each flag, in floats (every section is a multiple of 64 floats here but dw1c: al(513 * 64) = 32832)
_DEC_FLAG = 64
_PRN_FLAG = _DEC_FLAG + 64
_SCR_FLAG = _PRN_FLAG + 640 + 2 * 512 + 16 * 2 * 2 * 256 + 32832 + 128 * 128 + 256 * 128 + 512 * 256 + 64
FLAG_FROM_END = {"conv5_big": _SCR_FLAG, "dconv1a_big": _PRN_FLAG, "dconv2_inf": _DEC_FLAG, "dconv3_nan": _DEC_FLAG,
                 "dconv2_negzero": _DEC_FLAG, "dconv4_negzero": _DEC_FLAG, "conv4_big": 64}
PLANTS = {                                                  # plant -> (twin head, dtype)
    "conv5_big": ("ins_seg3", "fp32"), "dconv1a_big": ("ins_seg3", "fp32"), "dconv2_inf": ("ins_seg3", "fp32"),
    "dconv3_nan": ("ins_seg3", "fp32"), "dconv2_negzero": ("ins_seg3", "fp32"), "dconv4_negzero": ("ins_seg3", "fp32"),
    "conv4_big": ("static_box_est", "fp32"), "x3_overflow": ("ins_seg3", "f16x3"),
}
CASES = [f"{h}/{d}" for h in HEADS for d in DTYPES] + [f"{PLANTS[p][0]}/{PLANTS[p][1]}/{p}" for p in PLANTS]


def twin(case):
    """the clean case a planted case was copied from (None for a clean case)"""
    head, dtype, *plant = case.split("/")
    return f"{head}/{dtype}" if plant else None


_clean = {}


def clean_layers(head):
    """[{w (c_out, c_in), b, and with a BatchNorm gamma, beta, mean, var}] float32, built once per head"""
    if head not in _clean:
        out = []
        for name, bn, ci, co in HEADS[head][1]:
            rs = np.random.RandomState(zlib.crc32(f"{head}/{name}".encode()))
            L = {"w": (rs.standard_normal((co, ci)) / np.sqrt(ci)).astype(np.float32),
                 "b": (0.1 * rs.standard_normal(co)).astype(np.float32)}
            if bn:
                sign = np.where(rs.random_sample(co) < 0.5, -1.0, 1.0)
                L["gamma"] = (sign * rs.uniform(0.5, 1.5, co)).astype(np.float32)
                L["beta"] = (0.1 * rs.standard_normal(co) + 0.05).astype(np.float32)
                L["mean"] = (0.2 * rs.standard_normal(co) + 0.1).astype(np.float32)
                L["var"] = rs.uniform(0.5, 2.0, co).astype(np.float32)
                assert L["beta"].all() and L["mean"].all() and (sign < 0).any() and (sign > 0).any()
            out.append(L)
        _clean[head] = out
    return _clean[head]


def _negzero(L, ch):
    L["gamma"][ch] = -abs(L["gamma"][ch])
    L["b"][ch] = L["mean"][ch]
    L["beta"][ch] = -0.0


def layers(case):
    head, _, *plant = case.split("/")
    Ls = clean_layers(head)
    if not plant:
        return Ls
    Ls = [{k: v.copy() for k, v in L.items()} for L in Ls]
    p = plant[0]
    if p == "conv5_big":
        Ls[4]["w"][517, 33] = BIG
    elif p == "dconv1a_big":
        Ls[5]["w"][301, 41] = -BIG                          # a per-point column (< 64)
    elif p == "dconv2_inf":
        Ls[6]["w"][130, 257] = np.inf
    elif p == "dconv3_nan":
        Ls[7]["w"][77, 200] = np.nan
    elif p == "dconv2_negzero":
        _negzero(Ls[6], 201)
    elif p == "dconv4_negzero":
        _negzero(Ls[8], 5)
    elif p == "conv4_big":
        Ls[3]["w"][400, 100] = BIG
    elif p == "x3_overflow":
        Ls[2]["w"][9, 60] = BIG
    else:
        raise KeyError(case)
    return Ls


def pairs(case, device):
    """the case's (conv_or_linear, bn_or_None) pairs on `device`, in forward order"""
    head = case.split("/")[0]
    _, table, first_fc = HEADS[head]
    out = []
    with torch.no_grad():
        for i, ((name, bn, ci, co), L) in enumerate(zip(table, layers(case))):
            m = nn.Linear(ci, co) if i >= first_fc else nn.Conv1d(ci, co, 1)
            m.weight.copy_(torch.from_numpy(L["w"]).view_as(m.weight))
            m.bias.copy_(torch.from_numpy(L["b"]))
            b = None
            if bn:
                b = nn.BatchNorm1d(co)
                b.weight.copy_(torch.from_numpy(L["gamma"]))
                b.bias.copy_(torch.from_numpy(L["beta"]))
                b.running_mean.copy_(torch.from_numpy(L["mean"]))
                b.running_var.copy_(torch.from_numpy(L["var"]))
                b = b.to(device)
            out.append((m.to(device), b))
    return out


def pack(case, device="cuda"):
    """dal3_pack_weights on the case -> the blob's bytes (numpy uint8, on the host)"""
    head, dtype = case.split("/")[:2]
    ps = pairs(case, device)
    arr = (hip.Layer * len(ps))(*[hip.layer_struct(c, b) for c, b in ps])
    need = C.c_size_t(0)
    lib = hip.lib()
    hip.check(lib.dal3_pack_weights(HEADS[head][0], arr, len(ps), hip.DTYPES[dtype], None, C.byref(need), None))
    buf = torch.empty(need.value, dtype=torch.uint8, device=device)
    hip.check(lib.dal3_pack_weights(HEADS[head][0], arr, len(ps), hip.DTYPES[dtype], hip.ptr(buf), C.byref(need), hip.stream()))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def page_crcs(blob):
    b = blob.tobytes()
    return np.array([zlib.crc32(b[o:o + PAGE]) for o in range(0, len(b), PAGE)], np.uint32)


def flag_word(plant, blob):
    """the int32 of the guard flag that `plant` must set, read from an fp32 blob of the plant's head"""
    at = len(blob) - TAIL_BYTES - 4 * FLAG_FROM_END[plant]
    return int(blob[at:at + 4].view(np.int32)[0])
