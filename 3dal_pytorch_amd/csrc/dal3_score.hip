// dal3_score.hip — the baseline runs' scoring (dal3_score_tracks, dal3_best_gt_iou, include/dal3.h): the per-(track,
// frame) loop of the reference's tools/static_init.py:58-141,143-241 and tools/dynamic_init.py:37-123 — transform_box,
// the size2class / angle2class round trips, compute_box3d_iou, the threshold per type and the sums — from flat tables
// at any sample count, and the "best IoU over the frame's GT boxes" of tools/eval.py:72-87. The IoU of a pair is
// dal3_iou.hip's (the same device function, so dal3_box_iou_paired on the decoded float64 boxes gives the same bits).
//
// Sums: sample s belongs to chunk s / 256, whatever the grid. A chunk is reduced in a fixed order (the 64 lanes of a
// wave by a shuffle tree, the 4 waves in order) and its partial goes to the caller's slab with ordinary stores; a
// second one-workgroup launch adds the partials in a fixed order (thread t takes chunks t, t + 256, ... in sequence,
// then a fixed tree) and adds the result into the accumulator. The accumulator's bytes therefore depend on the input
// alone: not on the grid, not on the scheduling. No floating-point atomics.
#include "dal3_kernels.h"

// no FMA contraction: the decode must be the reference's float64 operations one by one, and the pair geometry the
// arithmetic of dal3_iou.hip's kernels (see dal3_iou.hip)
#pragma clang fp contract(off)

namespace {

#include "dal3_iou_pair.h"

constexpr int SC_BLOCK = 256;                   // = samples per chunk
constexpr int SC_WAVES = SC_BLOCK / 64;
constexpr int SC_COUNTS = 6;                    // pass, type 1, type 2, type 4, other type, scored

struct ScorePartial {                           // one chunk's sums (40 bytes)
    double bev, v3;
    uint32_t n[SC_COUNTS];
};

// class2size(*size2class(lwh)) of tools/utils.py:62-67,77-79: the class is np.argmin of np.linalg.norm(lwh - MEAN,
// axis=1) (the first minimum; a NaN is the minimum), the size MEAN[class] + (lwh - MEAN[class])
__device__ __forceinline__ void sc_size_round_trip(const double (&lwh)[3], double (&out)[3]) {
    int best = 0;
    double bv = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double dx = lwh[0] - mean_size_f64(c, 0), dy = lwh[1] - mean_size_f64(c, 1), dz = lwh[2] - mean_size_f64(c, 2);
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        if (c == 0) {
            bv = d;
        } else if (!(bv != bv) && (d != d || d < bv)) {
            best = c;
            bv = d;
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) out[j] = mean_size_f64(best, j) + (lwh[j] - mean_size_f64(best, j));
}

// a % b of NumPy / Python floats for b > 0 (npy_divmod): fmod, moved into [0, b) when negative
__device__ __forceinline__ double sc_mod(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) {
        if (m < 0.0) m += b;
    } else {
        m = 0.0;                                // copysign(0, b), b > 0
    }
    return m;
}

// class2angle(*angle2class(angle, 12), 12) of tools/utils.py:53-60,69-75 in float64; a non-finite angle gives NaN
__device__ __forceinline__ double sc_angle_round_trip(double angle) {
    if (!isfinite(angle)) return __builtin_nan("");
    const double two_pi = 2.0 * 3.141592653589793;
    const double per = two_pi / 12.0;
    angle = sc_mod(angle, two_pi);
    const double shifted = sc_mod(angle + per / 2.0, two_pi);
    const int cls = (int)(shifted / per);
    const double residual = shifted - ((double)cls * per + per / 2.0);
    double out = (double)cls * per + residual;
    if (out > 3.141592653589793) out = out - two_pi;
    return out;
}

__global__ __launch_bounds__(SC_BLOCK) void score_tracks_kernel(const dal3_score_args a, int64_t chunks,
                                                                ScorePartial* __restrict__ slab) {
    __shared__ double s_bev[SC_WAVES], s_3d[SC_WAVES];
    __shared__ uint32_t s_n[SC_WAVES][SC_COUNTS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double nan = __builtin_nan("");
    for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const int64_t s = chunk * SC_BLOCK + t;
        float vb = 0.f, v3 = 0.f;
        bool scored = false;
        int kind = 3;                           // 0, 1, 2: type 1, 2, 4; 3: any other
        if (s < a.S) {
            const int64_t r = a.box_row[s], f = a.frame[s];
            scored = a.has_gt[s] != 0 && r >= 0 && r < a.R && f >= 0 && f < a.F;
            double p[7], q[7];
            if (scored) {
                const double* b = a.boxes + 7 * r;
                const double* m = a.pose_inv + 16 * f;
                // transform_box (static_init.py:42-56): the 3x3 product summed in einsum's order, then the translation
#pragma unroll
                for (int i = 0; i < 3; ++i) p[i] = m[4 * i] * b[0] + m[4 * i + 1] * b[1] + m[4 * i + 2] * b[2] + m[4 * i + 3];
                const double init_yaw = b[6] + atan2(m[4], m[0]);
                const double lwh[3] = {b[3], b[4], b[5]};
                double size[3];
                sc_size_round_trip(lwh, size);
                p[3] = size[0];
                p[4] = size[1];
                p[5] = size[2];
                p[6] = 0.0;                     // class2angle(*angle2class(0)): class 0, residual 0.0
                double g[7];
#pragma unroll
                for (int j = 0; j < 7; ++j)
                    g[j] = a.gt_f64 ? static_cast<const double*>(a.gt)[7 * s + j]
                                    : (double)static_cast<const float*>(a.gt)[7 * s + j];
                const double glwh[3] = {g[3], g[4], g[5]};
                sc_size_round_trip(glwh, size);
                q[0] = g[0];                    // not rotated into the init box's frame: the reference's quirk
                q[1] = g[1];
                q[2] = g[2];
                q[3] = size[0];
                q[4] = size[1];
                q[5] = size[2];
                q[6] = sc_angle_round_trip(g[6] - init_yaw);
                box_iou_pair(iou_box<double>(p), iou_box<double>(q), vb, v3);
                const int ty = a.type[s];
                kind = ty == 1 ? 0 : ty == 2 ? 1 : ty == 4 ? 2 : 3;
            } else {
#pragma unroll
                for (int j = 0; j < 7; ++j) p[j] = q[j] = nan;
            }
            if (a.iou_bev) a.iou_bev[s] = scored ? vb : __builtin_nanf("");
            if (a.iou_3d) a.iou_3d[s] = scored ? v3 : __builtin_nanf("");
            if (a.pred_box) {
#pragma unroll
                for (int j = 0; j < 7; ++j) a.pred_box[7 * s + j] = p[j];
            }
            if (a.label_box) {
#pragma unroll
                for (int j = 0; j < 7; ++j) a.label_box[7 * s + j] = q[j];
            }
        }
        if (!slab) continue;                    // (uniform over the grid: no barrier is skipped by part of a block)
        const float thr = kind == 0 ? a.thr[0] : kind == 1 ? a.thr[1] : kind == 2 ? a.thr[2] : a.thr_other;
        double sum_bev = scored ? (double)vb : 0.0, sum_3d = scored ? (double)v3 : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {            // fixed pairing: the same order every run
            sum_bev += __shfl_down(sum_bev, off, 64);
            sum_3d += __shfl_down(sum_3d, off, 64);
        }
        const uint32_t n_pass = __popcll(__ballot(scored && v3 >= thr));
        const uint32_t n_k0 = __popcll(__ballot(scored && kind == 0)), n_k1 = __popcll(__ballot(scored && kind == 1));
        const uint32_t n_k2 = __popcll(__ballot(scored && kind == 2)), n_k3 = __popcll(__ballot(scored && kind == 3));
        const uint32_t n_scored = __popcll(__ballot(scored));
        if (lane == 0) {
            s_bev[wave] = sum_bev;
            s_3d[wave] = sum_3d;
            s_n[wave][0] = n_pass;
            s_n[wave][1] = n_k0;
            s_n[wave][2] = n_k1;
            s_n[wave][3] = n_k2;
            s_n[wave][4] = n_k3;
            s_n[wave][5] = n_scored;
        }
        __syncthreads();
        if (t == 0) {
            ScorePartial o;
            o.bev = ((s_bev[0] + s_bev[1]) + s_bev[2]) + s_bev[3];
            o.v3 = ((s_3d[0] + s_3d[1]) + s_3d[2]) + s_3d[3];
#pragma unroll
            for (int k = 0; k < SC_COUNTS; ++k) o.n[k] = s_n[0][k] + s_n[1][k] + s_n[2][k] + s_n[3][k];
            slab[chunk] = o;
        }
        __syncthreads();                        // s_* are free for the next chunk
    }
}

// stage two: one workgroup adds the chunks' partials in a fixed order and ADDS the result into the accumulator
__global__ __launch_bounds__(SC_BLOCK) void score_finish_kernel(const ScorePartial* __restrict__ slab, int64_t chunks,
                                                                int64_t S, dal3_score_acc* __restrict__ acc) {
    __shared__ double s_bev[SC_BLOCK], s_3d[SC_BLOCK];
    __shared__ unsigned long long s_n[SC_COUNTS][SC_BLOCK];
    const int t = threadIdx.x;
    double bev = 0.0, v3 = 0.0;
    unsigned long long n[SC_COUNTS] = {0, 0, 0, 0, 0, 0};
    for (int64_t c = t; c < chunks; c += SC_BLOCK) {
        bev += slab[c].bev;
        v3 += slab[c].v3;
#pragma unroll
        for (int k = 0; k < SC_COUNTS; ++k) n[k] += slab[c].n[k];
    }
    s_bev[t] = bev;
    s_3d[t] = v3;
#pragma unroll
    for (int k = 0; k < SC_COUNTS; ++k) s_n[k][t] = n[k];
    __syncthreads();
#pragma unroll
    for (int h = SC_BLOCK / 2; h > 0; h >>= 1) {
        if (t < h) {
            s_bev[t] += s_bev[t + h];
            s_3d[t] += s_3d[t + h];
#pragma unroll
            for (int k = 0; k < SC_COUNTS; ++k) s_n[k][t] += s_n[k][t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        acc->sum_iou_bev += s_bev[0];
        acc->sum_iou_3d += s_3d[0];
        acc->n_iou_3d_pass += s_n[0][0];
        acc->n_type[0] += s_n[1][0];
        acc->n_type[1] += s_n[2][0];
        acc->n_type[2] += s_n[3][0];
        acc->n_type[3] += s_n[4][0];
        acc->n_scored += s_n[5][0];
        acc->n_samples += (uint64_t)S;
    }
}

// ---------------------------------------------------------------------------------- best IoU over a frame's GT boxes
// One wave per query: the lanes stride the frame's GT range, each keeps its first maximum (np.argmax: a NaN is the
// maximum), and a shuffle tree merges the lanes with ties going to the lower index.
struct BestIou {
    float v3, bev;
    int32_t idx;                                // within the frame; INT32_MAX: nothing seen
};

__device__ __forceinline__ bool best_takes(const BestIou& cur, const BestIou& cand) {
    if (cand.idx == INT32_MAX) return false;
    if (cur.idx == INT32_MAX) return true;
    const bool cur_nan = cur.v3 != cur.v3, cand_nan = cand.v3 != cand.v3;
    if (cur_nan || cand_nan) return cand_nan && (!cur_nan || cand.idx < cur.idx);
    return cand.v3 > cur.v3 || (cand.v3 == cur.v3 && cand.idx < cur.idx);
}

template <typename T>
__global__ __launch_bounds__(SC_BLOCK) void best_gt_iou_kernel(const dal3_best_gt_args a) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * SC_WAVES;
    for (int64_t q = (int64_t)blockIdx.x * SC_WAVES + (threadIdx.x >> 6); q < a.Q; q += waves) {
        const int64_t f = a.query_frame[q];
        int64_t lo = 0, hi = 0;
        if (f >= 0 && f < a.F) {
            lo = a.gt_offsets[f];
            hi = a.gt_offsets[f + 1];
            lo = lo < 0 ? 0 : lo;
            hi = hi > a.G ? a.G : hi;
        }
        BestIou best = {0.f, 0.f, INT32_MAX};
        if (lo < hi) {
            const IouBox<T> qb = iou_box(static_cast<const T*>(a.queries) + 7 * q);
            for (int64_t j = lo + lane; j < hi; j += 64) {
                BestIou c;
                box_iou_pair(qb, iou_box(static_cast<const T*>(a.gt_boxes) + 7 * j), c.bev, c.v3);
                c.idx = (int32_t)(j - lo);
                if (best_takes(best, c)) best = c;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            BestIou o;
            o.v3 = __shfl_down(best.v3, off, 64);
            o.bev = __shfl_down(best.bev, off, 64);
            o.idx = __shfl_down(best.idx, off, 64);
            if (best_takes(best, o)) best = o;
        }
        if (lane == 0) {
            const bool none = best.idx == INT32_MAX;
            a.best_iou_3d[q] = none ? __builtin_nanf("") : best.v3;
            if (a.best_iou_bev) a.best_iou_bev[q] = none ? __builtin_nanf("") : best.bev;
            if (a.best_index) a.best_index[q] = none ? -1 : best.idx;
        }
    }
}

// workgroups of a grid-stride launch: all the work, up to 8 per CU of the CURRENT device (asked per call: a host-side
// table lookup, and a process that drives several devices gets each one's own count)
unsigned sc_grid(int64_t work, int64_t max_workgroups) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    int64_t g = work < 1 ? 1 : work;
    if (g > 8 * (int64_t)cus) g = 8 * (int64_t)cus;
    if (max_workgroups > 0 && g > max_workgroups) g = max_workgroups;
    return (unsigned)g;
}

}  // namespace

int64_t score_chunks(int64_t S) { return (S + SC_BLOCK - 1) / SC_BLOCK; }
size_t score_workspace_bytes(int64_t S) { return (size_t)score_chunks(S) * sizeof(ScorePartial); }

hipError_t launch_score_tracks(const dal3_score_args* a, hipStream_t s) {
    if (a->S <= 0) return hipSuccess;
    const int64_t chunks = score_chunks(a->S);
    ScorePartial* slab = a->acc ? static_cast<ScorePartial*>(a->workspace) : nullptr;
    hipLaunchKernelGGL(score_tracks_kernel, dim3(sc_grid(chunks, a->max_workgroups)), dim3(SC_BLOCK), 0, s, *a, chunks, slab);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !slab) return e;
    hipLaunchKernelGGL(score_finish_kernel, dim3(1), dim3(SC_BLOCK), 0, s, slab, chunks, a->S, a->acc);
    return hipGetLastError();
}

hipError_t launch_best_gt_iou(const dal3_best_gt_args* a, hipStream_t s) {
    if (a->Q <= 0) return hipSuccess;
    const dim3 grid(sc_grid((a->Q + SC_WAVES - 1) / SC_WAVES, a->max_workgroups));
    if (a->boxes_f64)
        hipLaunchKernelGGL(best_gt_iou_kernel<double>, grid, dim3(SC_BLOCK), 0, s, *a);
    else
        hipLaunchKernelGGL(best_gt_iou_kernel<float>, grid, dim3(SC_BLOCK), 0, s, *a);
    return hipGetLastError();
}
