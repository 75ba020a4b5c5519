"""tests/emu16.py — a MODEL of 16-bit MFMA arithmetic on the oracle's layers (test infrastructure, CPU, torch fp32).

VERDICT r5 #3: the 16-bit bars of tests/test_gpu_lowprec.py were "measured worst x <= 2" — derived from the product, so
they can neither catch a regression below 2x nor say whether 3e-2 is what bf16 SHOULD cost. This module states what the
arithmetic itself costs, independently of any kernel: the oracle's layers (oracle/ref_heads.py, which restates
tools/static_model.py:271-339 and tools/dynamic_model.py:187-312) with

  * eval-mode BatchNorm folded into the preceding weights (R.fold_bn), as every inference engine does,
  * the folded WEIGHTS and the layer's INPUT activations rounded to the 16-bit type (round-to-nearest-even) at every
    layer that include/dal3.h says runs on 16-bit MFMA operands: conv2..conv5, the per-point half of dconv1 and
    dconv2..dconv4 of the segmentation network (layer shapes: tools/dynamic_model.py:157-212), conv2..conv4 of the
    point heads,
  * products summed in fp32 (the MFMA's accumulator), biases added in fp32,
  * dconv5 (128 -> 2) likewise on 16-bit operands (the 16-bit decode kernel runs it as one more MFMA out-tile),
  * and everything else in fp32: the first layer (raw coordinates), the per-crop term of dconv1 (W1g . g + b1, a 1024-
    wide FC on the max-pooled feature), the max over points, the FC tails.

The tests then require  error(HIP 16-bit path) <= 1.5 x error(this model)  on the same rows, next to the absolute bars:
a kernel that loses more than the arithmetic must lose (a dropped rounding mode, a truncating conversion, a half-
precision accumulate) fails, however generous the absolute bar.
"""
import torch

from bound_model import fold as _fold
from oracle import ref_heads as R

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}     # ("fp32": no rounding — the structure check)
MODEL_SLACK = 1.5                                          # HIP error <= MODEL_SLACK x the model's error (maxima, mask-flip fractions)
RMS_SLACK = 1.15                                           # ... for rms errors (measured on MI355X, round 6: 0.98 - 1.01)


def q(x, prec):
    """round to the 16-bit type and back (RNE), exactly what a 16-bit MFMA operand holds"""
    return x.to(DT[prec]).float()


def _lin32(w, b, x):
    """(B,C,N) fp32 layer + ReLU"""
    return torch.relu(torch.einsum("oc,bcn->bon", w, x) + b[None, :, None])


def _lin16(w, b, x, prec, relu=True):
    """the same with 16-bit operands, fp32 accumulate, fp32 bias"""
    y = torch.einsum("oc,bcn->bon", q(w, prec), q(x, prec)) + b[None, :, None]
    return torch.relu(y) if relu else y


def ins_seg(sd, pts, prec, p="ins_seg"):
    """pts (B,Cin,N) fp32 -> logits (B,N,2): the segmentation network as 16-bit MFMA arithmetic computes it"""
    o1 = _lin32(*_fold(sd, p, "conv1", "bn1"), pts)
    o2 = _lin16(*_fold(sd, p, "conv2", "bn2"), o1, prec)
    o3 = _lin16(*_fold(sd, p, "conv3", "bn3"), o2, prec)
    o4 = _lin16(*_fold(sd, p, "conv4", "bn4"), o3, prec)
    o5 = _lin16(*_fold(sd, p, "conv5", "bn5"), o4, prec)
    g = o5.max(2)[0]                                                       # (B,1024) fp32
    w1, b1 = _fold(sd, p, "dconv1", "dbn1")                                # (512, 64 + 1024)
    crop_term = g @ w1[:, 64:].t() + b1                                    # fp32, per crop
    x = torch.relu(torch.einsum("oc,bcn->bon", q(w1[:, :64], prec), q(o2, prec)) + crop_term[:, :, None])
    x = _lin16(*_fold(sd, p, "dconv2", "dbn2"), x, prec)
    x = _lin16(*_fold(sd, p, "dconv3", "dbn3"), x, prec)
    x = _lin16(*_fold(sd, p, "dconv4", "dbn4"), x, prec)
    # dconv5 (128 -> 2, no BN / ReLU): in the 16-bit kernels a 17th out-tile of the decode stack, i.e. 16-bit operands too
    # (dal3_pointmlp_lp.hip); the fp32 kernels run it on the VALU
    return _lin16(*_fold(sd, p, "dconv5", None), x, prec, relu=False).transpose(2, 1).contiguous()


def point_head_pool(sd, p, x, prec):
    """conv1 (fp32) .. conv4 (16-bit operands) + max over points: (B,C,M) -> (B,512)"""
    x = _lin32(*_fold(sd, p, "conv1", "bn1"), x)
    for i in (2, 3, 4):
        x = _lin16(*_fold(sd, p, f"conv{i}", f"bn{i}"), x, prec)
    return x.max(2)[0]


def static_box_est(sd, obj, prec, p="box_est"):
    """(B,3,M) object points -> (B,39); the FC tail is fp32 (R's own layers)"""
    g = point_head_pool(sd, p, obj, prec)
    x = R._fbr(sd, p, "fc1", "fcbn1", g)
    x = R._fbr(sd, p, "fc2", "fcbn2", x)
    return torch.nn.functional.linear(x, sd[f"{p}.fc3.weight"], sd[f"{p}.fc3.bias"])


def embedding(sd, x, p, prec):
    g = point_head_pool(sd, p, x, prec)
    return R._fbr(sd, p, "fc2", "fcbn2", R._fbr(sd, p, "fc1", "fcbn1", g))


def rel(a, b):
    """max |a - b| / max |b| over everything (one number; the callers split parameter groups themselves where needed)"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


def rms(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b) ** 2).mean().sqrt() / b.abs().max())
