// dal3_fold.h — the BatchNorm fold of the detector's MFMA layers (include/dal3.h, "The fold"), written once: the dense
// stage's packer (dal3_conv2d.hip, which also packs every section of the RoI head's blob) and the sparse one
// (dal3_spconv.hip) call it, and tests/fold_ref.py restates it bit for bit.
//   scale = g / sqrt(var + eps)      W' = W * scale      b' = (b - mean) * scale + beta
// Every operation is a separately rounded float64 one (the _rn intrinsics: no contraction into an fma), the result is
// rounded once to float32. A layer without a BatchNorm has scale 1 and b' = b; one without a bias has b = 0.
//
// The pillar reader's pack (dal3_pillars.hip) is deliberately not on this header: its bias is written without pinned
// roundings, and moving it here could change its bits.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dal3.h"

struct FoldLayer {
    const float *w, *bias, *g, *beta, *mean, *var;
    int c_in, c_out;
    double eps;
    FoldLayer(const dal3_layer& l, double eps_)
        : w(l.weight), bias(l.bias), g(l.bn_weight), beta(l.bn_bias), mean(l.bn_mean), var(l.bn_var), c_in(l.c_in), c_out(l.c_out),
          eps(eps_) {}
};

__device__ __forceinline__ double fold_scale(const FoldLayer& L, int co) {
    return L.g ? (double)L.g[co] / __dsqrt_rn(__dadd_rn((double)L.var[co], L.eps)) : 1.0;
}

// b' of output channel co
__device__ __forceinline__ float fold_bias(const FoldLayer& L, int co) {
    const double b = L.bias ? (double)L.bias[co] : 0.0;
    return L.g ? (float)__dadd_rn(__dmul_rn(__dadd_rn(b, -(double)L.mean[co]), fold_scale(L, co)), (double)L.beta[co]) : (float)b;
}

// W' of the weight's element `at` (the packer's own layout), which belongs to output channel co
__device__ __forceinline__ float fold_weight(const FoldLayer& L, int64_t at, int co) {
    return (float)__dmul_rn((double)L.w[at], fold_scale(L, co));
}
