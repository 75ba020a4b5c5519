// dal3_center_loss.hip — the training side of CenterPoint's first stage (dal3_center_targets, dal3_center_loss of
// include/dal3.h, whose comment is the definition): AssignLabel's targets for every (sample, task) in one launch, and
// FastFocalLoss + RegLoss of one task with the gradients of every head map.
//
//   center_targets_kernel  a workgroup per (band of CT_ROWS map rows, task, sample). Every workgroup walks the sample's GT
//                          rows in order, ranks the rows of its task by ballot scans (block_rank: slot k is a function of
//                          the input alone) and keeps the live objects (cell, radius, class) in LDS. The heat map is then
//                          GATHERED: a pixel takes the maximum over the objects whose clipped square covers it, so no
//                          atomic and no zero fill is needed and the bits do not depend on scheduling. The first band's
//                          workgroup also writes the slots (anno_box, ind, mask, cat), zero rows included.
//   center_map_kernel      the negative focal term over the whole map: per-thread float64 sums in index order, a fixed
//                          tree per workgroup, one partial per workgroup; the gradient of every pixel, and the zero fill
//                          of the regression heads' gradient maps.
//   center_slot_kernel     a workgroup per sample: the positive focal term and the L1 terms of its slots (partials per
//                          sample), and the gradients at the slots' pixels. Slots that share a pixel are summed by the
//                          lowest slot among them, in ascending slot order, and written once.
//   center_final_kernel    one workgroup: the partials in a fixed order, the four results.
#include "dal3_block.h"
#include "dal3_kernels.h"
#pragma clang fp contract(off)

namespace {

constexpr int CT_BLOCK = 256, CT_WAVES = 4, CT_ROWS = 4;
constexpr int CL_BLOCK = 256, CL_PER_THREAD = 8, CL_CHUNK = CL_BLOCK * CL_PER_THREAD;
constexpr int CS_BLOCK = 512;
constexpr int CL_SUMS = 1 + DAL3_CENTER_MAX_COLS;        // per sample: the positive term, then the L1 sum of every column

// What the reference takes for the root of a r^2 - b r + c = 0: (b + sqrt(b^2 - 4 a c)) / 2, divided by 2 whatever a is
// (its quirk, kept).
__device__ __forceinline__ double radius_root(double a, double b, double c) { return (b + sqrt(b * b - 4.0 * a * c)) / 2.0; }

// The largest centre shift that keeps an IoU of `overlap` with a length x width box: the smallest of the three cases (one
// corner inward and one outward, both inward, both outward), float64.
__device__ __forceinline__ double gaussian_radius(double length, double width, double overlap) {
    const double side = length + width, area = width * length;
    const double mixed = radius_root(1.0, side, area * (1.0 - overlap) / (1.0 + overlap));
    const double inward = radius_root(4.0, 2.0 * side, (1.0 - overlap) * area);
    const double outward = radius_root(4.0 * overlap, -2.0 * overlap * side, (overlap - 1.0) * area);
    return fmin(mixed, fmin(inward, outward));
}

// numpy's float32 -> int32 cast where it is defined; anything else (a NaN, an infinity, beyond int32) is not a cell
__device__ __forceinline__ bool to_cell(float v, int32_t& out) {
    if (!(v > -2147483648.f && v < 2147483648.f)) return false;
    out = (int32_t)v;                               // toward zero
    return true;
}

__global__ __launch_bounds__(CT_BLOCK) void center_targets_kernel(const dal3_center_targets_args a) {
    __shared__ int32_t s_row[DAL3_CENTER_MAX_OBJS], s_cx[DAL3_CENTER_MAX_OBJS], s_cy[DAL3_CENTER_MAX_OBJS];
    __shared__ int32_t s_r[DAL3_CENTER_MAX_OBJS], s_cls[DAL3_CENTER_MAX_OBJS], s_list[DAL3_CENTER_MAX_OBJS];
    __shared__ int32_t s_cnt[CT_WAVES];

    const int t = threadIdx.x, task = blockIdx.y, b = blockIdx.z;
    const int H = (int)a.H, W = (int)a.W, G = (int)a.G, max_objs = a.max_objs;
    const int C = a.num_class[task];
    int class_base = 0;
    for (int i = 0; i < task; ++i) class_base += a.num_class[i];
    const int y0 = blockIdx.x * CT_ROWS;
    const bool first = blockIdx.x == 0;

    for (int k = t; k < max_objs; k += CT_BLOCK) s_row[k] = -1;
    __syncthreads();

    // ---- slot k of a row: its rank among the rows of this task, in row order
    const float* gt = a.gt + (int64_t)b * G * 10;
    int32_t base = 0;
    for (int g0 = 0; g0 < G; g0 += CT_BLOCK) {
        const int g = g0 + t;
        int cls = -1;
        if (g < G) {
            const float c = gt[(int64_t)g * 10 + 9];
            if (c > 0.f && c < 2147483000.f) cls = (int32_t)c - 1 - class_base;      // a NaN class is in no task
        }
        const bool mine = cls >= 0 && cls < C;
        int32_t total;
        const int32_t k = base + block_rank<CT_WAVES>(mine, s_cnt, total);
        base += total;
        if (!mine) continue;
        if (k >= max_objs) {
            if (first) atomicOr(a.status, DAL3_CENTER_OVERFLOW);
            continue;
        }
        const float* r = gt + (int64_t)g * 10;
        // every operation a float32 one, as on the reference's float32 range and size arrays
        const float wc = __fdiv_rn(__fdiv_rn(r[3], a.voxel_size[0]), a.out_size_factor);
        const float lc = __fdiv_rn(__fdiv_rn(r[4], a.voxel_size[1]), a.out_size_factor);
        if (!(wc > 0.f && lc > 0.f)) continue;
        double rad = gaussian_radius((double)lc, (double)wc, a.gaussian_overlap);
        if (!(rad < 65536.0)) rad = 65536.0;        // beyond any map (H, W <= 65535); a NaN as well
        const int32_t ri = (int32_t)rad;
        const float fx = __fdiv_rn(__fdiv_rn(__fsub_rn(r[0], a.pc_start[0]), a.voxel_size[0]), a.out_size_factor);
        const float fy = __fdiv_rn(__fdiv_rn(__fsub_rn(r[1], a.pc_start[1]), a.voxel_size[1]), a.out_size_factor);
        int32_t cx, cy;
        if (!to_cell(fx, cx) || !to_cell(fy, cy)) continue;
        if (cx < 0 || cx >= W || cy < 0 || cy >= H) continue;
        s_row[k] = g;
        s_cx[k] = cx;
        s_cy[k] = cy;
        s_r[k] = ri > a.min_radius ? ri : a.min_radius;
        s_cls[k] = cls;
    }
    __syncthreads();

    // ---- the objects whose square meets this band
    int32_t n_list = 0;
    for (int k0 = 0; k0 < max_objs; k0 += CT_BLOCK) {
        const int k = k0 + t;
        const bool hit = k < max_objs && s_row[k] >= 0 && s_cy[k] + s_r[k] >= y0 && s_cy[k] - s_r[k] < y0 + CT_ROWS;
        int32_t total;
        const int32_t at = n_list + block_rank<CT_WAVES>(hit, s_cnt, total);
        n_list += total;
        if (hit) s_list[at] = k;
    }
    __syncthreads();

    // ---- the band's pixels: exp(-(dx^2 + dy^2) / (2 sigma^2)), sigma = (2 r + 1) / 6, float64 rounded once; a maximum
    float* hm = a.hm[task] + (int64_t)b * C * H * W;
    const int band = CT_ROWS * W;
    for (int i = t; i < C * band; i += CT_BLOCK) {
        const int c = i / band, rem = i - c * band, y = y0 + rem / W, x = rem % W;
        if (y >= H) continue;
        float v = 0.f;
        for (int j = 0; j < n_list; ++j) {
            const int k = s_list[j];
            const int dx = x - s_cx[k], dy = y - s_cy[k], r = s_r[k];
            if (s_cls[k] != c || dx < -r || dx > r || dy < -r || dy > r) continue;
            const double sigma = (double)(2 * r + 1) / 6.0;
            const double d2 = (double)dx * (double)dx + (double)dy * (double)dy;
            v = fmaxf(v, (float)exp(-d2 / (2.0 * sigma * sigma)));
        }
        hm[((int64_t)c * H + y) * W + x] = v;
    }

    // ---- the slots
    if (!first) return;
    for (int k = t; k < max_objs; k += CT_BLOCK) {
        const int64_t o = (int64_t)b * max_objs + k;
        float* box = a.anno_box[task] + o * 10;
        const int g = s_row[k];
        if (g < 0) {
            for (int c = 0; c < 10; ++c) box[c] = 0.f;
            a.ind[task][o] = 0;
            a.mask[task][o] = 0;
            a.cat[task][o] = 0;
            continue;
        }
        const float* r = gt + (int64_t)g * 10;
        const float fx = __fdiv_rn(__fdiv_rn(__fsub_rn(r[0], a.pc_start[0]), a.voxel_size[0]), a.out_size_factor);
        const float fy = __fdiv_rn(__fdiv_rn(__fsub_rn(r[1], a.pc_start[1]), a.voxel_size[1]), a.out_size_factor);
        box[0] = __fsub_rn(fx, (float)s_cx[k]);     // exact: the fraction of a float32
        box[1] = __fsub_rn(fy, (float)s_cy[k]);
        box[2] = r[2];
        for (int c = 0; c < 3; ++c) box[3 + c] = (float)log((double)r[3 + c]);
        box[6] = r[7];
        box[7] = r[8];
        box[8] = (float)sin((double)r[6]);
        box[9] = (float)cos((double)r[6]);
        a.ind[task][o] = (int64_t)s_cy[k] * W + s_cx[k];
        a.mask[task][o] = 1;
        a.cat[task][o] = s_cls[k];
    }
}

// ------------------------------------------------------------------------------------------------ the loss

struct ClampedSigmoid {
    float p;        // clamp(sigmoid(x), 1e-4, 1 - 1e-4); a NaN stays one
    float ds;       // d p / d x: s (1 - s) where the clamp does not bind, else 0
};

__device__ __forceinline__ ClampedSigmoid clamped_sigmoid(float x) {
    const float lo = 1e-4f, hi = (float)(1.0 - 1e-4);
    const float s = __fdiv_rn(1.f, __fadd_rn(1.f, expf(-x)));
    ClampedSigmoid r;
    r.p = s < lo ? lo : (s > hi ? hi : s);
    r.ds = (s >= lo && s <= hi) ? __fmul_rn(s, __fsub_rn(1.f, s)) : 0.f;
    return r;
}

// log(1 - p) p^2 (1 - target)^4 and its derivative in p
__device__ __forceinline__ float neg_term(float p, float target, float& dp) {
    const float q = __fsub_rn(1.f, p), u = __fsub_rn(1.f, target);
    const float u2 = __fmul_rn(u, u), g = __fmul_rn(u2, u2);
    const float lq = logf(q), p2 = __fmul_rn(p, p);
    dp = __fmul_rn(g, __fsub_rn(__fmul_rn(__fmul_rn(2.f, p), lq), __fdiv_rn(p2, q)));
    return __fmul_rn(__fmul_rn(lq, p2), g);
}

// log(p) (1 - p)^2 and its derivative in p
__device__ __forceinline__ float pos_term(float p, float& dp) {
    const float q = __fsub_rn(1.f, p), lp = logf(p), q2 = __fmul_rn(q, q);
    dp = __fsub_rn(__fdiv_rn(q2, p), __fmul_rn(__fmul_rn(2.f, q), lp));
    return __fmul_rn(lp, q2);
}

__device__ __forceinline__ const float* map_at(const dal3_map& m, int64_t b, int64_t c, int64_t y, int64_t x) {
    return m.data + b * m.stride_b + c * m.stride_c + y * m.stride_h + x * m.stride_w;
}

// the sum of the task's mask over the batch, by every thread of the workgroup (an integer: exact in any order)
__device__ __forceinline__ int32_t mask_count(const uint8_t* mask, int64_t n, int32_t* s_count) {
    if (threadIdx.x == 0) *s_count = 0;
    __syncthreads();
    int32_t c = 0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) c += mask[i];
    if (c) atomicAdd(s_count, c);
    __syncthreads();
    return *s_count;
}

// -1 / num_pos, or -1 in the num_pos == 0 branch: d hm_loss / d (the negative sum)
__device__ __forceinline__ float hm_scale(int32_t num_pos) { return num_pos == 0 ? -1.f : __fdiv_rn(-1.f, (float)num_pos); }

struct LossWs {
    double* neg;        // one per workgroup of center_map_kernel
    double* sample;     // (B, CL_SUMS)
};

// indices are 32-bit here: B * (C + n_cols) * H * W < 2^31 (dal3_center_loss refuses anything larger)
__global__ __launch_bounds__(CL_BLOCK) void center_map_kernel(const dal3_center_loss_args a, LossWs ws, uint32_t n_hm, uint32_t n_reg) {
    __shared__ double s[CL_BLOCK];
    __shared__ int32_t s_count;
    const uint32_t t = threadIdx.x, Wd = (uint32_t)a.W;
    const uint32_t HW = (uint32_t)(a.H * a.W), CHW = a.C * HW, GHW = (a.C + a.n_cols) * HW;
    const float k = hm_scale(mask_count(a.mask, a.B * a.max_objs, &s_count));
    double sum = 0.0;
    const uint32_t i0 = blockIdx.x * (uint32_t)CL_CHUNK;
    for (int r = 0; r < CL_PER_THREAD; ++r) {
        const uint32_t i = i0 + (uint32_t)r * CL_BLOCK + t;
        if (i >= n_hm) break;
        const uint32_t b = i / CHW, rem = i - b * CHW, c = rem / HW, px = rem - c * HW, y = px / Wd, x = px - y * Wd;
        const ClampedSigmoid cs = clamped_sigmoid(*map_at(a.hm, b, c, y, x));
        float dp;
        sum += (double)neg_term(cs.p, a.target_hm[i], dp);
        a.grad[b * GHW + rem] = __fmul_rn(__fmul_rn(k, dp), cs.ds);
    }
    sum = block_sum_f64(sum, s, CL_BLOCK);
    if (t == 0) ws.neg[blockIdx.x] = sum;
    // this workgroup's share of the regression gradients' zero fill
    const uint32_t per = (n_reg + gridDim.x - 1) / gridDim.x, RHW = a.n_cols * HW;
    const uint32_t lo = per * blockIdx.x < n_reg ? per * blockIdx.x : n_reg, hi = n_reg - lo < per ? n_reg : lo + per;
    for (uint32_t i = lo + t; i < hi; i += CL_BLOCK) {
        const uint32_t b = i / RHW;
        a.grad[b * GHW + CHW + (i - b * RHW)] = 0.f;
    }
}

// column c of the regression target / prediction: which head map and which of its channels
__device__ __forceinline__ const float* reg_at(const dal3_center_loss_args& a, int c, int64_t b, int64_t y, int64_t x) {
    if (c < 2) return map_at(a.reg, b, c, y, x);
    if (c < 3) return map_at(a.height, b, 0, y, x);
    if (c < 6) return map_at(a.dim, b, c - 3, y, x);
    if (a.n_cols == 10 && c < 8) return map_at(a.vel, b, c - 6, y, x);
    return map_at(a.rot, b, c - (a.n_cols - 2), y, x);
}

__global__ __launch_bounds__(CS_BLOCK) void center_slot_kernel(const dal3_center_loss_args a, LossWs ws) {
    __shared__ double s[CS_BLOCK];
    __shared__ int32_t s_ind[DAL3_CENTER_MAX_OBJS], s_cat[DAL3_CENTER_MAX_OBJS];
    __shared__ float s_m[DAL3_CENTER_MAX_OBJS];
    __shared__ int32_t s_count;
    const int t = threadIdx.x, n = a.max_objs, cols = a.n_cols;
    const int64_t b = blockIdx.x, HW = a.H * a.W, CHW = a.C * HW, GHW = (a.C + cols) * HW;
    const int32_t num_pos = mask_count(a.mask, a.B * a.max_objs, &s_count);
    const float k_neg = hm_scale(num_pos), k_pos = num_pos == 0 ? 0.f : k_neg;      // num_pos == 0: the positive term is not in the graph
    const float den = __fadd_rn((float)num_pos, 1e-4f);

    for (int k = t; k < n; k += CS_BLOCK) {
        const int64_t o = b * n + k, ind = a.ind[o], cat = a.cat[o];
        const bool ok = ind >= 0 && ind < HW && cat >= 0 && cat < a.C;       // anything else is outside the contract: it is left out
        s_ind[k] = ok ? (int32_t)ind : -1;
        s_cat[k] = ok ? (int32_t)cat : -1;
        s_m[k] = ok ? (float)a.mask[o] : 0.f;
    }
    __syncthreads();

    // ---- this sample's sums: thread-strided in slot order, then the fixed tree
    double sums[CL_SUMS];
    for (int c = 0; c < CL_SUMS; ++c) sums[c] = 0.0;
    for (int k = t; k < n; k += CS_BLOCK) {
        if (s_ind[k] < 0) continue;
        const int64_t y = s_ind[k] / a.W, x = s_ind[k] - y * a.W;
        const float m = s_m[k];
        float dp;
        const float p = clamped_sigmoid(*map_at(a.hm, b, s_cat[k], y, x)).p;
        sums[0] += (double)__fmul_rn(pos_term(p, dp), m);
        const float* tgt = a.anno_box + (b * n + k) * 10;
        for (int c = 0; c < cols; ++c) {
            const float pred = *reg_at(a, c, b, y, x), tc = tgt[c < 6 ? c : c + (10 - cols)];
            sums[1 + c] += (double)fabsf(__fsub_rn(__fmul_rn(pred, m), __fmul_rn(tc, m)));
        }
    }
    for (int c = 0; c < 1 + cols; ++c) {
        const double v = block_sum_f64(sums[c], s, CS_BLOCK);
        if (t == 0) ws.sample[b * CL_SUMS + c] = v;
    }

    // ---- the gradients at the slots' pixels: the lowest slot of a pixel sums its peers in slot order and writes once
    for (int k = t; k < n; k += CS_BLOCK) {
        if (s_ind[k] < 0 || s_m[k] == 0.f) continue;
        const int ind = s_ind[k], cat = s_cat[k];
        bool own_px = true, own_hm = true;
        for (int j = 0; j < k; ++j) {
            if (s_ind[j] != ind || s_m[j] == 0.f) continue;
            own_px = false;
            if (s_cat[j] == cat) own_hm = false;
        }
        if (!own_hm) continue;                      // a pixel's owner owns its first class too
        const int64_t y = ind / a.W, x = ind - y * a.W;
        float* grad = a.grad + b * GHW + ind;
        {
            const ClampedSigmoid cs = clamped_sigmoid(*map_at(a.hm, b, cat, y, x));
            float dneg, dpos;
            neg_term(cs.p, a.target_hm[b * CHW + (int64_t)cat * HW + ind], dneg);
            pos_term(cs.p, dpos);
            float d = __fmul_rn(k_neg, dneg);
            for (int j = k; j < n; ++j)
                if (s_ind[j] == ind && s_cat[j] == cat && s_m[j] != 0.f) d = __fadd_rn(d, __fmul_rn(__fmul_rn(k_pos, dpos), s_m[j]));
            grad[(int64_t)cat * HW] = __fmul_rn(d, cs.ds);
        }
        if (!own_px) continue;
        for (int c = 0; c < cols; ++c) {
            const float pred = *reg_at(a, c, b, y, x);
            const float coef = __fdiv_rn(__fmul_rn(a.weight, a.code_weights[c]), den);
            float d = 0.f;
            for (int j = k; j < n; ++j) {
                if (s_ind[j] != ind || s_m[j] == 0.f) continue;
                const float m = s_m[j], tc = a.anno_box[(b * n + j) * 10 + (c < 6 ? c : c + (10 - cols))];
                const float diff = __fsub_rn(__fmul_rn(pred, m), __fmul_rn(tc, m));
                const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);     // 0 at 0, as l1_loss has it
                d = __fadd_rn(d, __fmul_rn(__fmul_rn(sgn, coef), m));
            }
            grad[(a.C + c) * HW] = d;
        }
    }
}

__global__ __launch_bounds__(CL_BLOCK) void center_final_kernel(const dal3_center_loss_args a, LossWs ws, int64_t n_blocks) {
    __shared__ double s[CL_BLOCK];
    __shared__ double s_tot[CL_SUMS];
    __shared__ int32_t s_count;
    const int t = threadIdx.x;
    const int32_t num_pos = mask_count(a.mask, a.B * a.max_objs, &s_count);
    double neg = 0.0;
    for (int64_t i = t; i < n_blocks; i += CL_BLOCK) neg += ws.neg[i];
    neg = block_sum_f64(neg, s, CL_BLOCK);
    if (t < 1 + a.n_cols) {
        double v = 0.0;
        for (int64_t b = 0; b < a.B; ++b) v += ws.sample[b * CL_SUMS + t];
        s_tot[t] = v;
    }
    __syncthreads();
    if (t != 0) return;
    const double hm_loss = num_pos == 0 ? -neg : -(s_tot[0] + neg) / (double)num_pos;
    const double den = (double)__fadd_rn((float)num_pos, 1e-4f);
    double loc = 0.0;
    for (int c = 0; c < a.n_cols; ++c) {
        const double e = s_tot[1 + c] / den;
        a.out[4 + c] = (float)e;
        loc += e * (double)a.code_weights[c];
    }
    a.out[0] = (float)(hm_loss + (double)a.weight * loc);
    a.out[1] = (float)hm_loss;
    a.out[2] = (float)loc;
    a.out[3] = (float)num_pos;
}

int64_t map_blocks(const dal3_center_loss_args* a) { return (a->B * a->C * a->H * a->W + CL_CHUNK - 1) / CL_CHUNK; }

LossWs carve_loss(Carver& c, const dal3_center_loss_args* a) {
    LossWs ws;
    ws.neg = c.take<double>((size_t)map_blocks(a));
    ws.sample = c.take<double>((size_t)a->B * CL_SUMS);
    return ws;
}

}  // namespace

hipError_t launch_center_targets(const dal3_center_targets_args* a, hipStream_t s) {
    if (a->B <= 0) return hipSuccess;
    const unsigned bands = (unsigned)((a->H + CT_ROWS - 1) / CT_ROWS);
    hipLaunchKernelGGL(center_targets_kernel, dim3(bands, (unsigned)a->T, (unsigned)a->B), dim3(CT_BLOCK), 0, s, *a);
    return hipGetLastError();
}

size_t center_loss_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W) {
    dal3_center_loss_args a = {};
    a.B = B, a.C = (int32_t)C, a.H = H, a.W = W;
    Carver c(nullptr, 0);
    carve_loss(c, &a);
    return c.off;
}

bool launch_center_loss(const dal3_center_loss_args* a, hipStream_t s, hipError_t* err) {
    Carver c(a->workspace, a->workspace_bytes);
    const LossWs ws = carve_loss(c, a);
    if (!c.ok) return false;
    const int64_t HW = a->H * a->W, blocks = map_blocks(a);
    hipLaunchKernelGGL(center_map_kernel, dim3((unsigned)blocks), dim3(CL_BLOCK), 0, s, *a, ws, (uint32_t)(a->B * a->C * HW), (uint32_t)(a->B * a->n_cols * HW));
    hipLaunchKernelGGL(center_slot_kernel, dim3((unsigned)a->B), dim3(CS_BLOCK), 0, s, *a, ws);
    hipLaunchKernelGGL(center_final_kernel, dim3(1), dim3(CL_BLOCK), 0, s, *a, ws, blocks);
    *err = hipGetLastError();
    return true;
}
