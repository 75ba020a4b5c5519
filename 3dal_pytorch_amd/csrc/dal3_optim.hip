// dal3_optim.hip — the detector's optimiser step (dal3_optim_grad_norm, dal3_optim_step, dal3_optim_total_norm of
// include/dal3.h, whose comment is the definition): Adam with decoupled ("true") or coupled weight decay, the gradient clip
// of clip_grad_norm_ and a one-cycle schedule table, for any number of parameters in two launches with nothing read back.
//
//   optim_norm_kernel   a workgroup per span of OPT_SPAN consecutive elements of the flat gradient buffer (the tensors'
//                       slices back to back, each padded with zeros to a multiple of 4): dwordx4 loads, per-thread float64
//                       sums of squares in index order, a fixed tree per workgroup, one partial per workgroup. Workgroup 0
//                       increments the step counter; nothing else here reads it.
//   optim_step_kernel   a workgroup per row of the chunk table (OPT_CHUNK elements of one tensor). Every workgroup reduces
//                       the partials for itself in one fixed order, so all of them hold the same bits of the norm and of
//                       the clip coefficient; thread 0 forms the step's scalars in float64 and the workgroup applies them.
//   optim_total_kernel  one workgroup: the same reduction, the norm as a float32 scalar.
//
// No floating-point atomic, no allocation, no host synchronisation: both launches can be captured in a hipGraph, and the
// replays walk the schedule by the device counter.
#include "dal3_block.h"
#include "dal3_kernels.h"
#pragma clang fp contract(off)

namespace {

constexpr int OPT_BLOCK = 256;
constexpr int OPT_CHUNK = DAL3_OPTIM_CHUNK;             // elements of one tensor per table row
constexpr int64_t OPT_SPAN = DAL3_OPTIM_NORM_SPAN;      // flat elements per partial sum
static_assert(OPT_CHUNK % (OPT_BLOCK * 4) == 0 && OPT_SPAN % (OPT_BLOCK * 4) == 0, "whole dwordx4 rounds per workgroup");

// sum of partials[0, n) in one fixed order (thread t takes t, t + OPT_BLOCK, ... ascending, then the fixed tree): every
// workgroup that calls it gets the same bits
__device__ __forceinline__ double reduce_partials(const double* partials, int64_t n, double* s_red) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += OPT_BLOCK) acc += partials[i];
    return block_sum_f64(acc, s_red, OPT_BLOCK);
}

__global__ __launch_bounds__(OPT_BLOCK) void optim_norm_kernel(const float* __restrict__ grad, int64_t n_flat, dal3_optim_hyper* hyper,
                                                               double* __restrict__ partials) {
    __shared__ double s_red[OPT_BLOCK];
    const int64_t lo = (int64_t)blockIdx.x * OPT_SPAN;
    double acc = 0.0;
    for (int64_t i = lo + (int64_t)threadIdx.x * 4; i < lo + OPT_SPAN && i + 4 <= n_flat; i += OPT_BLOCK * 4) {
        const float4 x = *reinterpret_cast<const float4*>(grad + i);
        acc += (double)x.x * (double)x.x;
        acc += (double)x.y * (double)x.y;
        acc += (double)x.z * (double)x.z;
        acc += (double)x.w * (double)x.w;
    }
    const double sum = block_sum_f64(acc, s_red, OPT_BLOCK);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = sum;
        if (blockIdx.x == 0) hyper->step = hyper->step + 1;
    }
}

__global__ __launch_bounds__(OPT_BLOCK) void optim_total_kernel(const double* __restrict__ partials, int64_t n_partials, float* out) {
    __shared__ double s_red[OPT_BLOCK];
    const double sum = reduce_partials(partials, n_partials, s_red);
    if (threadIdx.x == 0) *out = (float)sqrt(sum);
}

// what one step multiplies and adds with, float32 as torch's kernels take their Python scalars
struct StepScalars {
    float coef;             // the clip coefficient (1: the gradients keep their bits)
    float decay_mul;        // true_wd: 1 - wd lr
    float wd;               // coupled: g += wd p
    float w1, beta1;        // exp_avg: lerp weight 1 - beta1
    float beta2, w2;        // exp_avg_sq
    float bc2_sqrt, eps, neg_step_size;
    int clip, true_wd, fused_zero;
};

__device__ __forceinline__ float lerp_f32(float a, float b, float w) {     // torch's lerp
    return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.0f - w);
}

__global__ __launch_bounds__(OPT_BLOCK) void optim_step_kernel(const dal3_optim_chunk* __restrict__ chunks, float* __restrict__ grad,
                                                               float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                               int64_t n_flat, const double* __restrict__ partials,
                                                               int64_t n_partials, dal3_optim_hyper* hyper) {
    __shared__ double s_red[OPT_BLOCK];
    __shared__ StepScalars s_k;
    const int64_t flags = hyper->flags;
    double sumsq = 0.0;
    if (flags & DAL3_OPTIM_CLIP) sumsq = reduce_partials(partials, n_partials, s_red);
    if (threadIdx.x == 0) {
        StepScalars k;
        k.clip = (flags & DAL3_OPTIM_CLIP) != 0;
        k.true_wd = (flags & DAL3_OPTIM_TRUE_WD) != 0;
        k.fused_zero = (flags & DAL3_OPTIM_FUSED_ZERO) != 0;
        k.coef = 1.0f;
        if (k.clip) {                           // min(1, max_norm / (norm + 1e-6)); a NaN stays a NaN, as torch's clamp keeps it
            const double c = hyper->max_norm / (sqrt(sumsq) + 1e-6);
            k.coef = (float)(c > 1.0 ? 1.0 : c);
        }
        const int64_t step = hyper->step;
        double lr, beta1;
        const int64_t total = hyper->total_step;
        if (hyper->table && total > 0) {        // the block's own lr / beta1 are read by no workgroup then: workgroup 0 leaves
            int64_t row = step - 1 < total - 1 ? step - 1 : total - 1;     // the row it took there for the host to look at
            if (row < 0) row = 0;
            lr = hyper->table[2 * row];
            beta1 = hyper->table[2 * row + 1];
            if (blockIdx.x == 0) hyper->lr = lr, hyper->beta1 = beta1;
        } else {
            lr = hyper->lr, beta1 = hyper->beta1;
        }
        const double beta2 = hyper->beta2, wd = hyper->wd;
        const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
        k.decay_mul = (float)(1.0 - wd * lr);
        k.wd = (float)wd;
        k.w1 = (float)(1.0 - beta1);
        k.beta1 = (float)beta1;
        k.beta2 = (float)beta2;
        k.w2 = (float)(1.0 - beta2);
        k.bc2_sqrt = (float)sqrt(bc2);
        k.eps = (float)hyper->eps;
        k.neg_step_size = (float)(-(lr / bc1));
        s_k = k;
    }
    __syncthreads();
    const StepScalars k = s_k;
    const dal3_optim_chunk c = chunks[blockIdx.x];
    const int count = c.count;
    if (!c.param || c.offset < 0 || (c.offset & 3) || count < 1 || count > OPT_CHUNK || c.offset + ((count + 3) & ~3) > n_flat) return;
    float* p = c.param;
    const bool p_vec = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    const bool decay = c.decay != 0 && k.wd != 0.0f;
    for (int i = threadIdx.x * 4; i < count; i += OPT_BLOCK * 4) {
        const int64_t f = c.offset + i;
        const int live = count - i < 4 ? count - i : 4;     // the slice's pad lanes (zero in every flat buffer) stay zero
        const float4 g4 = *reinterpret_cast<const float4*>(grad + f);
        const float4 m4 = *reinterpret_cast<const float4*>(exp_avg + f);
        const float4 v4 = *reinterpret_cast<const float4*>(exp_avg_sq + f);
        float g[4] = {g4.x, g4.y, g4.z, g4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w}, w[4] = {0.f, 0.f, 0.f, 0.f};
        if (p_vec && live == 4) {
            const float4 w4 = *reinterpret_cast<const float4*>(p + i);
            w[0] = w4.x, w[1] = w4.y, w[2] = w4.z, w[3] = w4.w;
        } else {
            for (int e = 0; e < live; ++e) w[e] = p[i + e];
        }
        float g_out[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float ge = k.clip ? g[e] * k.coef : g[e];
            g_out[e] = e < live ? (k.fused_zero ? 0.0f : ge) : 0.0f;
            if (decay) {
                if (k.true_wd) w[e] = w[e] * k.decay_mul;
                else ge = ge + k.wd * w[e];
            }
            const float me = lerp_f32(m[e], ge, k.w1);
            const float ve = v[e] * k.beta2 + k.w2 * (ge * ge);
            const float denom = sqrtf(ve) / k.bc2_sqrt + k.eps;
            w[e] = w[e] + k.neg_step_size * (me / denom);
            m[e] = e < live ? me : 0.0f;
            v[e] = e < live ? ve : 0.0f;
        }
        *reinterpret_cast<float4*>(exp_avg + f) = make_float4(m[0], m[1], m[2], m[3]);
        *reinterpret_cast<float4*>(exp_avg_sq + f) = make_float4(v[0], v[1], v[2], v[3]);
        if (k.clip || k.fused_zero) *reinterpret_cast<float4*>(grad + f) = make_float4(g_out[0], g_out[1], g_out[2], g_out[3]);
        if (p_vec && live == 4) {
            *reinterpret_cast<float4*>(p + i) = make_float4(w[0], w[1], w[2], w[3]);
        } else {
            for (int e = 0; e < live; ++e) p[i + e] = w[e];
        }
    }
}

}  // namespace

int64_t optim_partials(int64_t n_flat) { return n_flat > 0 ? (n_flat + OPT_SPAN - 1) / OPT_SPAN : 0; }

hipError_t launch_optim_grad_norm(const float* grad, int64_t n_flat, dal3_optim_hyper* hyper, double* partials, hipStream_t s) {
    hipLaunchKernelGGL(optim_norm_kernel, dim3((unsigned)optim_partials(n_flat)), dim3(OPT_BLOCK), 0, s, grad, n_flat, hyper, partials);
    return hipGetLastError();
}

hipError_t launch_optim_step(const dal3_optim_chunk* chunks, int64_t n_chunks, float* grad, float* exp_avg, float* exp_avg_sq,
                             int64_t n_flat, const double* partials, dal3_optim_hyper* hyper, hipStream_t s) {
    hipLaunchKernelGGL(optim_step_kernel, dim3((unsigned)n_chunks), dim3(OPT_BLOCK), 0, s, chunks, grad, exp_avg, exp_avg_sq, n_flat,
                       partials, optim_partials(n_flat), hyper);
    return hipGetLastError();
}

hipError_t launch_optim_total_norm(const double* partials, int64_t n_partials, float* out, hipStream_t s) {
    hipLaunchKernelGGL(optim_total_kernel, dim3(1), dim3(OPT_BLOCK), 0, s, partials, n_partials, out);
    return hipGetLastError();
}
