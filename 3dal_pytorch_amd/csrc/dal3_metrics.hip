// dal3_metrics.hip — box-estimation training metrics (dal3_box_estimation_metrics, include/dal3.h): the per-step
// compute_box3d_iou of the reference's train / eval loops (tools/utils.py:81-103) plus the accumulation around it, in
// one launch. The IoU of a pair is dal3_iou.hip's (the same device function, so dal3_box_iou_paired on the decoded
// float64 boxes gives the same bits).
#include "dal3_kernels.h"

// no FMA contraction: the decode must be the reference's float64 operations one by one, and the pair geometry the
// arithmetic of dal3_iou.hip's kernels (see dal3_iou.hip)
#pragma clang fp contract(off)

namespace {

#include "dal3_iou_pair.h"

// ---------------------------------------------------------------------------------- box-estimation training metrics
// dal3_box_estimation_metrics (include/dal3.h). Block 0 owns every per-item term: it decodes and scores the B pairs
// (a thread takes items t, t + 256, ...) and reduces the float sums in a fixed tree, so the batch's sums have one
// order whatever the scheduling — bitwise reproducible without a slab. Blocks 1.. count the segmentation term, one
// (item, 1024-point chunk) each, and add their integer count with one atomic.
constexpr int BM_BLOCK = 256;
constexpr int BM_PTS = 4;                       // points per thread of a segmentation block
constexpr int BM_CHUNK = BM_BLOCK * BM_PTS;

__device__ __forceinline__ double bm_ld(const void* p, int64_t i, int f64) {
    return f64 ? static_cast<const double*>(p)[i] : (double)static_cast<const float*>(p)[i];
}

__device__ __forceinline__ int64_t bm_ldi(const void* p, int64_t i, int i32) {
    return i32 ? (int64_t)static_cast<const int32_t*>(p)[i] : static_cast<const int64_t*>(p)[i];
}

// np.argmax / torch.argmax over K values of one row: the first index of the maximum; a NaN is the maximum (the first)
template <int K>
__device__ __forceinline__ int bm_argmax(const void* p, int64_t row, int f64) {
    int best = 0;
    double bv = bm_ld(p, row, f64);
#pragma unroll
    for (int k = 1; k < K; ++k) {
        const double v = bm_ld(p, row + k, f64);
        if (!(bv != bv) && (v != v || v > bv)) {
            best = k;
            bv = v;
        }
    }
    return best;
}

// [cx, cy, cz, l, w, h, yaw] of class2angle / class2size; an out-of-range class gives NaN and reads nothing
__device__ __forceinline__ void bm_box(const void* center, int64_t c_row, int c_f64, int64_t hc, const void* hres,
                                       int64_t h_at, int h_f64, int64_t sc, const void* sres, int64_t s_at, int s_f64,
                                       double (&box)[7]) {
    const double per = 2.0 * 3.141592653589793 / 12.0;
    const double nan = __builtin_nan("");
#pragma unroll
    for (int j = 0; j < 3; ++j) box[j] = bm_ld(center, c_row + j, c_f64);
    if (hc >= 0 && hc < 12) {
        double a = (double)hc * per + bm_ld(hres, h_at, h_f64);
        if (a > 3.141592653589793) a = a - 2.0 * 3.141592653589793;
        box[6] = a;
    } else {
        box[6] = nan;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) box[3 + j] = (sc >= 0 && sc < 3) ? mean_size_f64((int)sc, j) + bm_ld(sres, s_at + j, s_f64) : nan;
}

__global__ __launch_bounds__(BM_BLOCK) void box_estimation_metrics_kernel(const dal3_box_metric_args a, int64_t chunks) {
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        __shared__ double s_bev[BM_BLOCK], s_3d[BM_BLOCK];
        __shared__ unsigned s_pass[BM_BLOCK];
        const int F = a.f64_fields, I = a.i32_fields;
        double sum_bev = 0.0, sum_3d = 0.0;
        unsigned pass = 0;
        for (int64_t k = t; k < a.B; k += BM_BLOCK) {
            double p[7], q[7];
            const int hc = bm_argmax<12>(a.heading_scores, k * a.ld_heading_scores, F & DAL3_BM_HEADING_SCORES);
            const int sc = bm_argmax<3>(a.size_scores, k * a.ld_size_scores, F & DAL3_BM_SIZE_SCORES);
            bm_box(a.center, k * a.ld_center, F & DAL3_BM_CENTER, hc, a.heading_residuals, k * a.ld_heading_residuals + hc,
                   F & DAL3_BM_HEADING_RESIDUALS, sc, a.size_residuals, k * a.ld_size_residuals + 3 * sc,
                   F & DAL3_BM_SIZE_RESIDUALS, p);
            const int64_t hcl = bm_ldi(a.heading_class_label, k * a.ld_heading_class_label, I & DAL3_BM_HEADING_CLASS_LABEL);
            const int64_t scl = bm_ldi(a.size_class_label, k * a.ld_size_class_label, I & DAL3_BM_SIZE_CLASS_LABEL);
            bm_box(a.center_label, k * a.ld_center_label, F & DAL3_BM_CENTER_LABEL, hcl, a.heading_residual_label,
                   k * a.ld_heading_residual_label, F & DAL3_BM_HEADING_RESIDUAL_LABEL, scl, a.size_residual_label,
                   k * a.ld_size_residual_label, F & DAL3_BM_SIZE_RESIDUAL_LABEL, q);
            float vb, v3;
            box_iou_pair(iou_box<double>(p), iou_box<double>(q), vb, v3);
            if (a.iou_bev) a.iou_bev[k] = vb;
            if (a.iou_3d) a.iou_3d[k] = v3;
            sum_bev += (double)vb;
            sum_3d += (double)v3;
            pass += v3 >= a.thr ? 1u : 0u;
        }
        if (!a.acc) return;                     // (uniform over the block: no barrier is skipped by part of it)
        s_bev[t] = sum_bev;
        s_3d[t] = sum_3d;
        s_pass[t] = pass;
        __syncthreads();
#pragma unroll
        for (int h = BM_BLOCK / 2; h > 0; h >>= 1) {     // fixed pairing: the same order every run
            if (t < h) {
                s_bev[t] += s_bev[t + h];
                s_3d[t] += s_3d[t + h];
                s_pass[t] += s_pass[t + h];
            }
            __syncthreads();
        }
        if (t == 0) {
            a.acc->sum_iou_bev += s_bev[0];
            a.acc->sum_iou_3d += s_3d[0];
            if (a.loss) a.acc->sum_loss += (double)*a.loss;
            a.acc->n_iou_3d_pass += s_pass[0];
            a.acc->n_items += (uint64_t)a.B;
        }
        return;
    }
    // segmentation: item b, points [n0, n0 + BM_CHUNK)
    const int64_t blk = (int64_t)blockIdx.x - 1;
    const int64_t b = blk / chunks, n0 = (blk - b * chunks) * BM_CHUNK;
    const float* lg = a.logits + b * a.logits_stride_b;
    unsigned correct = 0;
#pragma unroll
    for (int i = 0; i < BM_PTS; ++i) {
        const int64_t n = n0 + i * BM_BLOCK + t;
        if (n < a.N) {
            const float l0 = lg[n * a.logits_stride_n], l1 = lg[n * a.logits_stride_n + a.logits_stride_c];
            const int64_t pred = (l0 != l0) ? 0 : ((l1 != l1) ? 1 : (l1 > l0 ? 1 : 0));
            const int64_t at = b * a.mask_stride_b + n * a.mask_stride_n;
            int64_t lab;
            if (a.mask_dtype == DAL3_MASK_F32) {
                const float v = static_cast<const float*>(a.mask_label)[at];
                lab = (v > -9.2e18f && v < 9.2e18f) ? (int64_t)v : -1;      // NaN / out of int64 range: no match
            } else {
                lab = static_cast<const uint8_t*>(a.mask_label)[at];
            }
            correct += pred == lab ? 1u : 0u;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) correct += __shfl_down(correct, off, 64);
    __shared__ unsigned s_wave[BM_BLOCK / 64];
    if ((t & 63) == 0) s_wave[t >> 6] = correct;
    __syncthreads();
    if (t == 0) {
        unsigned long long c = 0;
#pragma unroll
        for (int w = 0; w < BM_BLOCK / 64; ++w) c += s_wave[w];
        if (c) atomicAdd(reinterpret_cast<unsigned long long*>(&a.acc->n_seg_correct), c);
    }
}

}  // namespace

int64_t box_estimation_metrics_chunks(int64_t N) { return (N + BM_CHUNK - 1) / BM_CHUNK; }

hipError_t launch_box_estimation_metrics(const dal3_box_metric_args* a, hipStream_t s) {
    const int64_t chunks = a->logits ? box_estimation_metrics_chunks(a->N) : 0;
    const int64_t blocks = 1 + (a->logits ? a->B * chunks : 0);
    if (blocks == 1 && a->B == 0 && !(a->acc && a->loss)) return hipSuccess;   // nothing to score or add
    hipLaunchKernelGGL(box_estimation_metrics_kernel, dim3((unsigned)blocks), dim3(BM_BLOCK), 0, s, *a,
                       chunks > 0 ? chunks : 1);
    return hipGetLastError();
}
