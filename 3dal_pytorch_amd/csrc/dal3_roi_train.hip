// dal3_roi_train.hip — the training side of CenterPoint's second stage (dal3_roi_targets, dal3_roi_loss of include/dal3.h,
// whose comment is the definition): ProposalTargetLayer.forward + RoIHeadTemplate.assign_targets for every sample in one
// launch, and the two RoI losses with their gradients in another.
//
//   roi_targets_kernel   one workgroup of 512 threads per sample. Thread m < M holds slot m (the fused form resolves it with
//                        dal3_roi_head's own walk, dal3_roi_slots.h), trims the GT list (the last non-zero row: an integer
//                        maximum), scores the slot against the GT rows of its class (dal3_iou_pair.h, ascending g, a strict
//                        `>`: the lowest index among the maxima), and enters one of the three ordered lists (fg, hard bg,
//                        easy bg) by block_rank, so a list is ascending in m whatever the hardware does. The fg permutation
//                        is a rank sort of (key[p], p) in LDS: position p counts the pairs below it, no two ranks are
//                        equal, no atomic decides a position. Thread j < R then reads its sampled slot and writes row j.
//   roi_loss_kernel      one workgroup: every thread sums its rows in index order in float64, the partial sums meet in a
//                        fixed tree; a second pass over the rows writes the gradients with the counts known.
#include "dal3_block.h"
#include "dal3_kernels.h"
#include "dal3_roi_slots.h"
#pragma clang fp contract(off)

namespace {

#include "dal3_iou_pair.h"

constexpr int RT_BLOCK = 512, RT_WAVES = 8;     // DAL3_ROI_TRAIN_MAX_M = DAL3_ROI_TRAIN_MAX_R = RT_BLOCK
constexpr int RL_BLOCK = 256;
static_assert(DAL3_ROI_TRAIN_MAX_M == RT_BLOCK && DAL3_ROI_TRAIN_MAX_R == RT_BLOCK, "one thread per slot and per sampled row");

// torch's `%` on float32 (the result takes the divisor's sign)
__device__ __forceinline__ float remainder_f(float x, float p) {
    float r = fmodf(x, p);
    if (r != 0.f && ((r < 0.f) != (p < 0.f))) r = __fadd_rn(r, p);
    return r;
}

// the c-th with-replacement draw from a list of n > 0: min(int(pick * n), n - 1), the product a float32 one; a pick outside
// [0, 1) (outside the contract) still lands inside the list
__device__ __forceinline__ int draw_at(float pick, int n) {
    const float v = __fmul_rn(pick, (float)n);
    int i = v >= 0.f ? (v < (float)n ? (int)v : n - 1) : 0;      // a NaN lands on 0
    return i < n - 1 ? i : n - 1;
}

__global__ __launch_bounds__(RT_BLOCK) void roi_targets_kernel(const dal3_roi_targets_args a) {
    __shared__ float s_roi[RT_BLOCK * 9];
    __shared__ float s_score[RT_BLOCK], s_iou[RT_BLOCK], s_key[RT_BLOCK];
    __shared__ int32_t s_label[RT_BLOCK], s_asg[RT_BLOCK], s_live[RT_BLOCK];
    __shared__ int32_t s_fg[RT_BLOCK], s_hard[RT_BLOCK], s_easy[RT_BLOCK], s_perm[RT_BLOCK];
    __shared__ int32_t s_cnt[RT_WAVES];
    __shared__ int32_t s_last;

    const int t = threadIdx.x, b = blockIdx.x;
    const int M = (int)a.M, R = (int)a.R, G = (int)a.G, code = a.code_size;
    if (t == 0) s_last = 0;
    s_perm[t] = t;                                  // a NaN key (outside the contract) leaves valid positions behind

    // ---- the slot
    float roi[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float score = 0.f;
    int32_t label = 0, live = 0;
    if (t < M) {
        if (a.keep) {
            int64_t before, row;
            int task, bad;
            roi_slot_row(a.keep, a.keep_count, a.seg_offsets, a.T, (int)a.B, a.K, a.keep_stride, b, t, before, row, task, bad);
            if (t == 0 && before > M) atomicOr(a.status, DAL3_ROI_OVERFLOW);
            if (bad) atomicOr(a.status, DAL3_NMS_BAD_SEGMENT);
            if (row >= 0) {
                const float* box = a.boxes + row * code;
                for (int c = 0; c < 6; ++c) roi[c] = box[c];
                roi[6] = box[code - 1];
                for (int c = 7; c < code; ++c) roi[c] = box[c - 1];
                score = a.scores[row];
                label = a.labels[row] + a.label_base[task] + 1;
                live = 1;
            }
        } else {
            const int64_t i = (int64_t)b * M + t;
            for (int c = 0; c < code; ++c) roi[c] = a.rois[i * code + c];
            score = a.roi_scores[i];
            label = a.roi_labels[i];
            live = label != 0;
        }
    }
    for (int c = 0; c < 9; ++c) s_roi[t * 9 + c] = roi[c];
    s_score[t] = score;
    s_label[t] = label;
    s_live[t] = live;
    s_key[t] = t < M ? a.draws[(int64_t)b * (M + R) + t] : 0.f;
    __syncthreads();                                // s_last is zero for everyone

    // ---- the GT trim: the last row with a non-zero entry, row 0 at the least
    const float* gt = a.gt + (int64_t)b * G * (code + 1);
    int last = 0;
    for (int g = t; g < G; g += RT_BLOCK) {
        bool any = false;
        for (int c = 0; c <= code; ++c) any = any || gt[(int64_t)g * (code + 1) + c] != 0.f;     // a NaN counts
        if (any) last = g;
    }
    if (last > 0) atomicMax(&s_last, last);         // an integer maximum: the order does not matter
    __syncthreads();
    const int n_gt = s_last + 1;

    // ---- get_max_iou_with_same_class without the class loop
    float best = 0.f;
    int32_t asg = 0;
    if (t < M) {
        bool found = false;
        const IouBox<float> q = iou_box<float>(roi);
        for (int g = 0; g < n_gt; ++g) {
            const float* row = gt + (int64_t)g * (code + 1);
            const float cls = row[code];
            if (!(fabsf(cls) < 2147483000.f) || (int32_t)cls != label) continue;      // .long() truncates; a NaN class matches nothing
            float bev, v3, v;
            box_iou_pair(q, iou_box<float>(row), bev, v3, &v);
            // torch.max: the first of the maxima, and a NaN wins (the first NaN)
            if (!found || v > best || (v != v && best == best)) {
                best = v;
                asg = g;
                found = true;
            }
        }
    }
    s_iou[t] = best;
    s_asg[t] = asg;

    // ---- the three ascending lists
    const float fg_thresh = fminf(a.reg_fg_thresh, a.cls_fg_thresh);
    const bool is_fg = t < M && best >= fg_thresh;
    const bool is_easy = t < M && best < a.cls_bg_thresh_lo;
    const bool is_hard = t < M && best < a.reg_fg_thresh && best >= a.cls_bg_thresh_lo;
    int32_t n_fg, n_hard, n_easy;
    const int32_t r_fg = block_rank<RT_WAVES>(is_fg, s_cnt, n_fg);
    const int32_t r_hard = block_rank<RT_WAVES>(is_hard, s_cnt, n_hard);
    const int32_t r_easy = block_rank<RT_WAVES>(is_easy, s_cnt, n_easy);
    if (is_fg) s_fg[r_fg] = t;
    if (is_hard) s_hard[r_hard] = t;
    if (is_easy) s_easy[r_easy] = t;
    __syncthreads();

    // ---- the fg permutation: positions ordered by (key[p], p)
    if (t < n_fg) {
        const float k = s_key[t];
        int32_t rank = 0;
        for (int q = 0; q < n_fg; ++q) {
            const float kq = s_key[q];
            rank += (kq < k || (kq == k && q < t)) ? 1 : 0;
        }
        s_perm[rank < n_fg ? rank : n_fg - 1] = t;  // ranks are distinct for keys without a NaN
    }
    __syncthreads();

    // ---- row j of the output
    if (t >= R) return;
    const int j = t;
    const float* pick = a.draws + (int64_t)b * (M + R) + M;
    const int n_bg = n_hard + n_easy;
    int m = -1;
    {
        int c = j, bg_n = R;                        // the c-th of bg_n background rows
        bool bg = n_bg > 0;
        if (n_fg > 0 && n_bg > 0) {
            const int fg_this = a.fg_per_image < n_fg ? a.fg_per_image : n_fg;
            if (j < fg_this) {
                m = s_fg[s_perm[j]];
                bg = false;
            }
            c = j - fg_this;
            bg_n = R - fg_this;
        } else if (n_fg > 0) {
            m = s_fg[draw_at(pick[j], n_fg)];
            bg = false;
        }
        if (bg) {
            if (n_hard > 0 && n_easy > 0) {
                const int cap = (int)((double)bg_n * a.hard_bg_ratio);
                const int hn = cap < n_hard ? cap : n_hard;
                m = c < hn ? s_hard[draw_at(pick[c], n_hard)] : s_easy[draw_at(pick[c], n_easy)];
            } else if (n_hard > 0) {
                m = s_hard[draw_at(pick[c], n_hard)];
            } else {
                m = s_easy[draw_at(pick[c], n_easy)];
            }
        }
    }
    const int64_t o = (int64_t)b * R + j;
    const bool none = m < 0;                        // neither fg nor bg: NaN overlaps
    if (none) {
        if (j == 0) atomicOr(a.status, DAL3_ROI_NO_SAMPLE);
        m = 0;
    }
    const float* r = s_roi + m * 9;
    const float* src = gt + (int64_t)s_asg[m] * (code + 1);
    const float iou = none ? 0.f : s_iou[m];
    const int32_t smp = (!none && s_live[m]) ? b : -1;
    a.slot[o] = m;
    a.sample[o] = smp;
    for (int c = 0; c < code; ++c) a.out_rois[o * code + c] = none ? 0.f : r[c];
    a.out_labels[o] = none ? 0 : s_label[m];
    a.out_scores[o] = none ? 0.f : s_score[m];
    a.gt_iou[o] = iou;
    a.reg_valid[o] = iou > a.reg_fg_thresh ? 1 : 0;
    float lab;
    if (a.cls_score_type == DAL3_ROI_CLS_SCORE_CLS) {
        lab = iou > a.cls_fg_thresh ? 1.f : 0.f;
        if (iou > a.cls_bg_thresh && iou < a.cls_fg_thresh) lab = -1.f;
    } else {
        const bool fgm = iou > a.cls_fg_thresh, bgm = iou < a.cls_bg_thresh;
        lab = fgm ? 1.f : 0.f;
        if (!fgm && !bgm) lab = __fdiv_rn(__fsub_rn(iou, a.cls_bg_thresh), a.cls_thresh_span);
    }
    a.cls_labels[o] = lab;
    // the sampled box with the rotation back in the last column: dal3_box_points' layout
    {
        float* bx = a.out_boxes + o * code;
        for (int c = 0; c < 6; ++c) bx[c] = none ? 0.f : r[c];
        for (int c = 7; c < code; ++c) bx[c - 1] = none ? 0.f : r[c];
        bx[code - 1] = none ? 0.f : r[6];
    }
    // assign_targets' encoding, every operation a float32 one in the reference's order
    float* enc = a.gt_of_rois + o * (code + 1);
    float* raw = a.gt_src + o * (code + 1);
    if (none) {
        for (int c = 0; c <= code; ++c) enc[c] = raw[c] = 0.f;
        return;
    }
    const float two_pi = 6.283185307179586f, pi = 3.141592653589793f, half_pi = 1.5707963267948966f, pi15 = 4.71238898038469f;
    float gsrc[10], e[10];
    for (int c = 0; c <= code; ++c) raw[c] = gsrc[c] = src[c];
    const float ry = __fsub_rn(r[6], __fmul_rn(floorf(__fadd_rn(__fdiv_rn(r[6], two_pi), 0.5f)), two_pi));
    for (int c = 0; c < 6; ++c) e[c] = __fsub_rn(gsrc[c], r[c]);
    e[6] = __fsub_rn(gsrc[6], ry);
    for (int c = 7; c <= code; ++c) e[c] = gsrc[c];
    const float ang = -ry, ca = cosf(ang), sa = sinf(ang);
    const float x = __fadd_rn(__fmul_rn(e[0], ca), __fmul_rn(e[1], sa));
    const float y = __fadd_rn(__fmul_rn(e[0], -sa), __fmul_rn(e[1], ca));
    e[0] = x;
    e[1] = y;
    for (int c = 7; c < code; ++c) e[c] = __fsub_rn(e[c], r[c]);     // the velocity's difference, not rotated
    float h = remainder_f(e[6], two_pi);
    if (h > half_pi && h < pi15) h = remainder_f(__fadd_rn(h, pi), two_pi);
    if (h > pi) h = __fsub_rn(h, two_pi);
    h = fminf(fmaxf(h, -half_pi), half_pi);
    e[6] = h;
    for (int c = 0; c <= code; ++c) enc[c] = e[c];
}

struct LossGeom {
    const float *cls, *reg, *labels, *target;
    const int32_t* valid;
    int64_t N;
    int code;
    float cw[9], cls_w, reg_w;
    float *loss, *d_cls, *d_reg;
};

__global__ __launch_bounds__(RL_BLOCK) void roi_loss_kernel(const LossGeom g) {
    __shared__ double s[RL_BLOCK];
    const int t = threadIdx.x;
    double cls_sum = 0.0, reg_sum = 0.0, n_cls = 0.0, n_fg = 0.0;
    for (int64_t i = t; i < g.N; i += RL_BLOCK) {
        const float y = g.labels[i];
        if (y >= 0.f) {
            const float p = __fdiv_rn(1.f, __fadd_rn(1.f, expf(-g.cls[i])));
            const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(logf(__fsub_rn(1.f, p)), -100.f);
            cls_sum += (double)(-__fadd_rn(__fmul_rn(y, lp), __fmul_rn(__fsub_rn(1.f, y), lq)));
            n_cls += 1.0;
        }
        if (g.valid[i] > 0) {
            n_fg += 1.0;
            for (int c = 0; c < g.code; ++c)
                reg_sum += (double)__fmul_rn(fabsf(__fsub_rn(g.reg[i * g.code + c], g.target[i * (g.code + 1) + c])), g.cw[c]);
        }
    }
    cls_sum = block_sum_f64(cls_sum, s, RL_BLOCK);
    reg_sum = block_sum_f64(reg_sum, s, RL_BLOCK);
    n_cls = block_sum_f64(n_cls, s, RL_BLOCK);
    n_fg = block_sum_f64(n_fg, s, RL_BLOCK);
    const double dc = n_cls > 1.0 ? n_cls : 1.0, df = n_fg > 1.0 ? n_fg : 1.0;
    if (t == 0) {
        const float lc = (float)(cls_sum / dc) * g.cls_w, lr = (float)(reg_sum / df) * g.reg_w;
        g.loss[0] = lc;
        g.loss[1] = lr;
        g.loss[2] = __fadd_rn(lc, lr);
    }
    const float kc = g.cls_w / (float)dc, kr = g.reg_w / (float)df;
    for (int64_t i = t; i < g.N; i += RL_BLOCK) {
        const float y = g.labels[i];
        float d = 0.f;
        if (y >= 0.f) {
            // binary_cross_entropy's backward ((p - y) / max(p (1 - p), 1e-12)) through the sigmoid's (p (1 - p))
            const float p = __fdiv_rn(1.f, __fadd_rn(1.f, expf(-g.cls[i])));
            const float pq = __fmul_rn(p, __fsub_rn(1.f, p));
            d = __fmul_rn(__fmul_rn(__fdiv_rn(__fsub_rn(p, y), fmaxf(pq, 1e-12f)), pq), kc);
        }
        g.d_cls[i] = d;
        const bool fg = g.valid[i] > 0;
        for (int c = 0; c < g.code; ++c) {
            const float diff = __fsub_rn(g.reg[i * g.code + c], g.target[i * (g.code + 1) + c]);
            const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);     // 0 at 0; a NaN gives 0
            g.d_reg[i * g.code + c] = fg ? __fmul_rn(__fmul_rn(sgn, g.cw[c]), kr) : 0.f;
        }
    }
}

}  // namespace

hipError_t launch_roi_targets(const dal3_roi_targets_args* a, hipStream_t s) {
    if (a->B <= 0) return hipSuccess;
    hipLaunchKernelGGL(roi_targets_kernel, dim3((unsigned)a->B), dim3(RT_BLOCK), 0, s, *a);
    return hipGetLastError();
}

hipError_t launch_roi_loss(const float* rcnn_cls, const float* rcnn_reg, int64_t N, int code_size, const float* cls_labels,
                           const int32_t* reg_valid, const float* gt_of_rois, const float* code_weights, float cls_weight,
                           float reg_weight, float* loss, float* d_cls, float* d_reg, hipStream_t s) {
    LossGeom g = {};
    g.cls = rcnn_cls, g.reg = rcnn_reg, g.labels = cls_labels, g.target = gt_of_rois, g.valid = reg_valid;
    g.N = N, g.code = code_size;
    for (int c = 0; c < code_size; ++c) g.cw[c] = code_weights[c];
    g.cls_w = cls_weight, g.reg_w = reg_weight;
    g.loss = loss, g.d_cls = d_cls, g.d_reg = d_reg;
    hipLaunchKernelGGL(roi_loss_kernel, dim3(1), dim3(RL_BLOCK), 0, s, g);
    return hipGetLastError();
}
