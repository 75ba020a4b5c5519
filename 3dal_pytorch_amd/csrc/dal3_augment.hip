// dal3_augment.hip — the detector's training input on the device (include/dal3.h, "The training input"): ground-truth paste
// from the object database with the reference's collision test and greedy acceptance (DataBaseSamplerV2.sample_class_v2,
// box_collision_test), the global flip / rotation / scaling / translation and the shuffle of the points in one pass
// (Preprocess.__call__, det3d/core/sampler/preprocess.py), and the boxes' side of the same transforms with
// filter_gt_box_outside_range, limit_period and AssignLabel's regrouping into gt_boxes_and_cls.
//
// Every decision that the reference takes in float32 is taken here in float32, one rounding per operation: the file is
// compiled without contraction and the products of a comparison are written as separate roundings.
#include "dal3_block.h"
#include "dal3_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int AUG_BLOCK = 256;
constexpr int AUG_WAVES = AUG_BLOCK / 64;
// The pair matrix lives in LDS as one 64-bit word per box (bit i: candidate i collides with this box) beside the box's
// four BEV corners: 8 + 32 = 40 bytes a box. 1024 boxes take 40 KiB of the 64 KiB a workgroup may declare statically and
// leave room for the candidates' groups; the next power of two would not fit.
static_assert(DAL3_AUG_MAX_BOXES * 40 + DAL3_AUG_MAX_CAND * 4 + 64 <= 65536, "the pair matrix must fit the static LDS budget");
static_assert(DAL3_AUG_MAX_CAND == 64, "one 64-bit word holds a box's column of the pair matrix");

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }

// center_to_corner_box2d(box[0:2], box[3:5], box[8]) in float32: corners_nd's clockwise corners (-,-), (-,+), (+,+), (+,-)
// of half the size, rotation_2d's x' = x cos + y sin, y' = -x sin + y cos, then the centre. c: x0, y0, x1, y1, ...
__device__ __forceinline__ void bev_corners(float x, float y, float w, float l, float rot, float* c) {
    const float sn = (float)sin((double)rot), cs = (float)cos((double)rot);
    const float nx[4] = {-0.5f, -0.5f, 0.5f, 0.5f}, ny[4] = {-0.5f, 0.5f, 0.5f, -0.5f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float px = mul(w, nx[k]), py = mul(l, ny[k]);
        c[2 * k] = add(add(mul(px, cs), mul(py, sn)), x);
        c[2 * k + 1] = add(add(mul(px, -sn), mul(py, cs)), y);
    }
}

// box_collision_test's entry [box, qbox]: stand-up overlap (strict), the sixteen edge pairs, the two containment loops
__device__ bool collide(const float* a, const float* q) {
    float a0 = a[0], a1 = a[1], a2 = a[0], a3 = a[1], q0 = q[0], q1 = q[1], q2 = q[0], q3 = q[1];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        a0 = fminf(a0, a[2 * k]), a1 = fminf(a1, a[2 * k + 1]), a2 = fmaxf(a2, a[2 * k]), a3 = fmaxf(a3, a[2 * k + 1]);
        q0 = fminf(q0, q[2 * k]), q1 = fminf(q1, q[2 * k + 1]), q2 = fmaxf(q2, q[2 * k]), q3 = fmaxf(q3, q[2 * k + 1]);
    }
    if (!(sub(fminf(a2, q2), fmaxf(a0, q0)) > 0.f)) return false;
    if (!(sub(fminf(a3, q3), fmaxf(a1, q1)) > 0.f)) return false;
    for (int k = 0; k < 4; ++k) {
        const float Ax = a[2 * k], Ay = a[2 * k + 1], Bx = a[2 * ((k + 1) & 3)], By = a[2 * ((k + 1) & 3) + 1];
        for (int l = 0; l < 4; ++l) {
            const float Cx = q[2 * l], Cy = q[2 * l + 1], Dx = q[2 * ((l + 1) & 3)], Dy = q[2 * ((l + 1) & 3) + 1];
            const bool acd = mul(sub(Dy, Ay), sub(Cx, Ax)) > mul(sub(Cy, Ay), sub(Dx, Ax));
            const bool bcd = mul(sub(Dy, By), sub(Cx, Bx)) > mul(sub(Cy, By), sub(Dx, Bx));
            if (acd != bcd) {
                const bool abc = mul(sub(Cy, Ay), sub(Bx, Ax)) > mul(sub(By, Ay), sub(Cx, Ax));
                const bool abd = mul(sub(Dy, Ay), sub(Bx, Ax)) > mul(sub(By, Ay), sub(Dx, Ax));
                if (abc != abd) return true;
            }
        }
    }
    // every corner of `in` strictly inside `out` (clockwise edges, cross >= 0 is outside)
    auto inside = [](const float* out, const float* in) {
        for (int l = 0; l < 4; ++l)
            for (int k = 0; k < 4; ++k) {
                const float vx = -sub(out[2 * k], out[2 * ((k + 1) & 3)]), vy = -sub(out[2 * k + 1], out[2 * ((k + 1) & 3) + 1]);
                const float cross = sub(mul(vy, sub(out[2 * k], in[2 * l])), mul(vx, sub(out[2 * k + 1], in[2 * l + 1])));
                if (cross >= 0.f) return false;
            }
        return true;
    };
    return inside(a, q) || inside(q, a);
}

// one workgroup per sample
__global__ __launch_bounds__(AUG_BLOCK) void paste_select_kernel(dal3_gt_paste_args a) {
    __shared__ float s_c[DAL3_AUG_MAX_BOXES][8];
    __shared__ unsigned long long s_m[DAL3_AUG_MAX_BOXES];
    __shared__ int32_t s_group[DAL3_AUG_MAX_CAND];
    const int b = blockIdx.x, t = threadIdx.x;
    const int64_t nc64 = a.cand_counts[b];
    const int32_t ng32 = a.gt_counts[b];
    uint8_t* accept = a.accept + (int64_t)b * a.max_cand;
    if (nc64 < 0 || nc64 > a.max_cand || nc64 > DAL3_AUG_MAX_CAND || ng32 < 0 || ng32 > a.max_gt || ng32 + nc64 > DAL3_AUG_MAX_BOXES) {
        for (int i = t; i < a.max_cand; i += AUG_BLOCK) accept[i] = 0;
        if (t == 0) atomicOr(a.status, DAL3_AUG_TOO_MANY);
        return;
    }
    const int nc = (int)nc64, ng = ng32, n = ng + nc;
    for (int j = t; j < n; j += AUG_BLOCK) {
        const float* box = j < ng ? a.gt_boxes + ((int64_t)b * a.max_gt + j) * 9 : a.cand_boxes + ((int64_t)b * a.max_cand + (j - ng)) * 9;
        bev_corners(box[0], box[1], box[3], box[4], box[8], s_c[j]);
        if (j >= ng) s_group[j - ng] = (int32_t)a.cand_group[(int64_t)b * a.max_cand + (j - ng)];
    }
    __syncthreads();
    // thread j holds box j's column: candidate i's row entry [i, j] is bit i. A GT box whose class is negative (a name the
    // reference drops before it samples) collides with nothing; the diagonal is left out.
    for (int j = t; j < n; j += AUG_BLOCK) {
        unsigned long long m = 0;
        const bool dead = j < ng && a.gt_classes[(int64_t)b * a.max_gt + j] < 0;
        if (!dead)
            for (int i = 0; i < nc; ++i)
                if (ng + i != j && collide(s_c[ng + i], s_c[j])) m |= 1ull << i;
        s_m[j] = m;
        if (a.coll)
            for (int i = 0; i < nc; ++i)
                a.coll[((int64_t)b * a.max_cand + i) * (a.max_gt + a.max_cand) + (j < ng ? j : a.max_gt + (j - ng))] = (m >> i) & 1;
    }
    __syncthreads();
    if (t >= 64) return;
    // the reference's serial loop on one wave: candidate i is tested against the GT boxes, the earlier groups' accepted
    // boxes and its own group's boxes that are not rejected yet; a rejected box's row and column are dead from then on
    unsigned long long accepted = 0, rejected = 0;
    for (int i = 0; i < nc; ++i) {
        const int g = s_group[i];
        bool hit = false;
        for (int j = t; j < n; j += 64) {
            bool live = true;
            if (j >= ng) {
                const int c = j - ng, gc = s_group[c];
                live = gc < g ? ((accepted >> c) & 1) : gc == g ? !((rejected >> c) & 1) : false;
            }
            hit |= live && ((s_m[j] >> i) & 1);
        }
        if (__ballot(hit)) rejected |= 1ull << i;
        else accepted |= 1ull << i;
    }
    for (int i = t; i < a.max_cand; i += 64) accept[i] = i < nc ? (uint8_t)((accepted >> i) & 1) : 0;
}

// ------------------------------------------------------------------------------------------------ points
struct SampleXf {                               // one sample's transform, (B) of them in the workspace
    float sn, cs, scale;
    int32_t flip_y, flip_x;
    float pad[3];
};

// the composite (sample, order key) of every source row, and the samples' transforms
__global__ __launch_bounds__(AUG_BLOCK) void augment_prep_kernel(dal3_augment_points_args a, uint64_t* key, SampleXf* xf) {
    const int64_t i0 = (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x;
    for (int64_t b = i0; a.transform && b < a.B; b += (int64_t)gridDim.x * AUG_BLOCK) {
        const double* d = a.xform + b * 7;
        SampleXf x = {};
        x.flip_y = d[0] != 0.0, x.flip_x = d[1] != 0.0;
        x.sn = (float)sin(d[2]), x.cs = (float)cos(d[2]), x.scale = (float)d[3];
        xf[b] = x;
    }
    if (!key) return;
    for (int64_t i = i0; i < a.n; i += (int64_t)gridDim.x * AUG_BLOCK) {
        const int64_t b = upper_bound(a.out_offsets, (int64_t)0, a.B + 1, i) - 1;
        key[i] = ((uint64_t)b << 32) | (uint64_t)(a.keys[i] & 0x7fffffff);
    }
}

// output row p <- source row pos[p] (p itself without a shuffle): one read, the transform, one write
template <int F>
__global__ __launch_bounds__(AUG_BLOCK) void augment_points_kernel(dal3_augment_points_args a, const int32_t* pos, const SampleXf* xf) {
    const float nan = __int_as_float(0x7fc00000);
    for (int64_t p = (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x; p < a.n; p += (int64_t)gridDim.x * AUG_BLOCK) {
        const int64_t b = upper_bound(a.out_offsets, (int64_t)0, a.B + 1, p) - 1;
        const int64_t s = pos ? pos[p] : p, lo = a.out_offsets[b], hi = a.out_offsets[b + 1];
        float v[F];
        bool ok = s >= lo && s < hi, pasted = false;
        const float* src = nullptr;
        int64_t k = 0;
        if (ok) {
            const int64_t nc = a.cand_counts[b], c0 = b * a.max_cand;
            const int64_t cand_end = nc > 0 ? a.cand_seg_start[c0 + nc - 1] + a.cand_rows[c0 + nc - 1] : lo;
            if (s < cand_end) {
                k = upper_bound(a.cand_seg_start, c0, c0 + nc, s) - 1;
                const int64_t r = a.cand_db_row[k] + (s - a.cand_seg_start[k]);
                ok = k >= c0 && r >= 0 && r < a.db_rows;
                pasted = true;
                src = a.db_points + r * F;
            } else {
                const int64_t r = a.scene_offsets[b] + (s - cand_end);
                ok = r >= 0 && r < a.n_scene;
                src = a.scene + r * F;
            }
        }
        if (!ok) atomicOr(a.status, DAL3_AUG_BAD_ROW);
        if (ok && pasted && !a.accept[k]) ok = false;          // a rejected object's row: NaN, which dal3_voxelize drops
        if (ok) {
            if (F == 4) {
                const float4 q = *reinterpret_cast<const float4*>(src);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < F; ++j) v[j] = src[j];
            }
            if (pasted) {
                const float* box = a.cand_boxes + k * 9;
                v[0] = add(v[0], box[0]), v[1] = add(v[1], box[1]), v[2] = add(v[2], box[2]);
            }
            if (a.transform) {
                const SampleXf x = xf[b];
                const double* tr = a.xform + b * 7 + 4;
                if (x.flip_y) v[1] = -v[1];
                if (x.flip_x) v[0] = -v[0];
                const float rx = add(mul(v[0], x.cs), mul(v[1], x.sn)), ry = add(mul(v[0], -x.sn), mul(v[1], x.cs));
                // the reference adds its float64 draw to the float32 points: the sum is formed in float64 and rounded once
                v[0] = (float)((double)mul(rx, x.scale) + tr[0]);
                v[1] = (float)((double)mul(ry, x.scale) + tr[1]);
                v[2] = (float)((double)mul(v[2], x.scale) + tr[2]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < F; ++j) v[j] = nan;
        }
        float* dst = a.out + p * F;
        if (F == 4) {
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < F; ++j) dst[j] = v[j];
        }
    }
}

int sort_passes(int64_t B) {                    // 31 bits of order key, then the sample
    int p = 4;
    for (int64_t top = B - 1; top > 0; top >>= 8) ++p;
    return p;
}

struct AugWs {
    RadixBufs<uint64_t> radix;
    SampleXf* xf;
    size_t bytes;
    bool ok;
};

AugWs carve_augment(void* base, size_t size, int64_t B, int64_t n) {
    Carver c(base, size);
    AugWs w = {};
    w.xf = c.take<SampleXf>((size_t)(B > 0 ? B : 1));
    w.radix = carve_radix<uint64_t>(c, n > 0 ? n : 1, 2);
    w.bytes = c.off;
    w.ok = c.ok;
    return w;
}

// ------------------------------------------------------------------------------------------------ boxes
__device__ __forceinline__ bool corner_in_range(float px, float py, const float* poly) {
    // points_in_convex_polygon_jit on minmax_to_corner_2d's polygon: edge k runs from corner k - 1 to corner k
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = (k + 3) & 3;
        const float vx = sub(poly[2 * k], poly[2 * j]), vy = sub(poly[2 * k + 1], poly[2 * j + 1]);
        const float cross = sub(mul(vy, sub(poly[2 * k], px)), mul(vx, sub(poly[2 * k + 1], py)));
        if (cross >= 0.f) return false;
    }
    return true;
}

// one workgroup per sample
__global__ __launch_bounds__(AUG_BLOCK) void augment_boxes_kernel(dal3_augment_boxes_args a) {
    __shared__ int32_t s_cnt[AUG_WAVES];
    __shared__ int32_t s_cls[DAL3_AUG_MAX_BOXES];       // the kept box's class, 0: dropped
    __shared__ float s_box[DAL3_AUG_MAX_BOXES][10];     // its output row, parked until its rank is known
    const int b = blockIdx.x, t = threadIdx.x;
    float* out = a.out + (int64_t)b * a.max_objs * 10;
    for (int i = t; i < a.max_objs * 10; i += AUG_BLOCK) out[i] = 0.f;
    const int64_t nc64 = a.accept ? a.cand_counts[b] : 0;
    const int32_t ng = a.gt_counts[b];
    if (nc64 < 0 || nc64 > a.max_cand || ng < 0 || ng > a.max_gt || ng + nc64 > DAL3_AUG_MAX_BOXES) {
        if (t == 0) atomicOr(a.status, DAL3_AUG_TOO_MANY), a.out_count[b] = 0;
        return;
    }
    const int nc = (int)nc64, n = ng + nc;
    // minmax_to_corner_2d(range): the minimum plus (0, 0), (0, dy), (dx, dy), (dx, 0), in float32
    const float dx = sub(a.range[2], a.range[0]), dy = sub(a.range[3], a.range[1]);
    const float poly[8] = {add(mul(dx, 0.f), a.range[0]), add(mul(dy, 0.f), a.range[1]), add(mul(dx, 0.f), a.range[0]), add(dy, a.range[1]),
                           add(dx, a.range[0]), add(dy, a.range[1]), add(dx, a.range[0]), add(mul(dy, 0.f), a.range[1])};
    const double zero7[7] = {0, 0, 0, 1, 0, 0, 0};
    const double* d = a.transform ? a.xform + (int64_t)b * 7 : zero7;
    const float pi = 3.14159274101257324f, two_pi = 6.28318548202514648f;       // float32(np.pi), float32(2 * np.pi)
    for (int j = t; j < n; j += AUG_BLOCK) {
        const bool gt = j < ng;
        const int64_t row = gt ? (int64_t)b * a.max_gt + j : (int64_t)b * a.max_cand + (j - ng);
        const float* src = (gt ? a.gt_boxes : a.cand_boxes) + row * 9;
        const int64_t cls = gt ? (int64_t)a.gt_classes[row] : a.cand_classes[row];
        bool keep = cls >= 1 && cls <= a.n_classes && (gt || a.accept[row]);
        float v[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] = src[k];
        if (a.transform) {
            if (d[0] != 0.0) v[1] = -v[1], v[8] = add(-v[8], pi), v[7] = -v[7];
            if (d[1] != 0.0) v[0] = -v[0], v[8] = add(-v[8], two_pi), v[6] = -v[6];
            const float sn = (float)sin(d[2]), cs = (float)cos(d[2]);
            const float rx = add(mul(v[0], cs), mul(v[1], sn)), ry = add(mul(v[0], -sn), mul(v[1], cs));
            // the velocities go through a float64 product in the reference (hstack with float64 zeros)
            const double sn64 = sin(d[2]), cs64 = cos(d[2]);
            const float ux = (float)__dadd_rn(__dmul_rn((double)v[6], cs64), __dmul_rn((double)v[7], sn64));
            const float uy = (float)__dadd_rn(__dmul_rn((double)v[6], -sn64), __dmul_rn((double)v[7], cs64));
            v[0] = rx, v[1] = ry, v[6] = ux, v[7] = uy;
            v[8] = add(v[8], (float)d[2]);
            const float sc = (float)d[3];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = mul(v[k], sc);
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = (float)((double)v[k] + d[4 + k]);
        }
        if (keep) {
            float c[8];
            bev_corners(v[0], v[1], v[3], v[4], v[8], c);
            bool any = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) any |= corner_in_range(c[2 * k], c[2 * k + 1], poly);
            keep = any;
        }
        s_cls[j] = keep ? (int32_t)cls : 0;
        if (keep) {
            float* w = s_box[j];
            v[8] = sub(v[8], mul(floorf(add(__fdiv_rn(v[8], two_pi), 0.5f)), two_pi));      // limit_period(rot, 0.5, 2 pi)
            w[0] = v[0], w[1] = v[1], w[2] = v[2], w[3] = v[3], w[4] = v[4], w[5] = v[5], w[6] = v[8], w[7] = v[6], w[8] = v[7];
            w[9] = (float)cls;
        }
    }
    __syncthreads();
    // AssignLabel's order: by class (the tasks partition the class list in order), the rows of a class in input order
    int32_t base = 0;
    for (int c = 1; c <= a.n_classes; ++c)
        for (int j0 = 0; j0 < n; j0 += AUG_BLOCK) {
            const int j = j0 + t;
            const bool mine = j < n && s_cls[j] == c;
            int32_t total;
            const int32_t r = base + block_rank<AUG_WAVES>(mine, s_cnt, total);
            if (mine && r < a.max_objs) {
#pragma unroll
                for (int k = 0; k < 10; ++k) out[(int64_t)r * 10 + k] = s_box[j][k];
            }
            base += total;
        }
    if (t == 0) {
        a.out_count[b] = base < a.max_objs ? base : a.max_objs;
        if (base > a.max_objs) atomicOr(a.status, DAL3_AUG_OVERFLOW);
    }
}

}  // namespace

hipError_t launch_gt_paste_select(const dal3_gt_paste_args* a, hipStream_t s) {
    if (a->B == 0) return hipSuccess;
    hipLaunchKernelGGL(paste_select_kernel, dim3((unsigned)a->B), dim3(AUG_BLOCK), 0, s, *a);
    return hipGetLastError();
}

size_t augment_points_workspace_bytes(int64_t B, int64_t n) { return carve_augment(nullptr, 0, B, n).bytes; }

bool launch_augment_points(const dal3_augment_points_args* a, hipStream_t s, hipError_t* err) {
    *err = hipSuccess;
    const AugWs w = carve_augment(a->workspace, a->workspace_bytes, a->B, a->n);
    if (!w.ok) return false;
    if (a->n == 0 || a->B == 0) return true;
    const bool sorted = a->keys != nullptr;
    const unsigned grid = grid_clamp((a->n + AUG_BLOCK - 1) / AUG_BLOCK, 65536, a->max_workgroups);
    hipLaunchKernelGGL(augment_prep_kernel, dim3(grid), dim3(AUG_BLOCK), 0, s, *a, sorted ? w.radix.key[0] : (uint64_t*)nullptr, w.xf);
    const int32_t* pos = nullptr;
    if (sorted) {
        const int passes = sort_passes(a->B);
        *err = radix_sort_pairs(w.radix, a->n, passes, grid_clamp(radix_chunks(a->n), 65536, a->max_workgroups), s);
        if (*err != hipSuccess) return true;
        pos = w.radix.pos[passes & 1];
    }
    switch (a->F) {
#define AUG_CASE(F_) \
    case F_: hipLaunchKernelGGL(augment_points_kernel<F_>, dim3(grid), dim3(AUG_BLOCK), 0, s, *a, pos, (const SampleXf*)w.xf); break;
        AUG_CASE(3) AUG_CASE(4) AUG_CASE(5) AUG_CASE(6) AUG_CASE(7) AUG_CASE(8)
#undef AUG_CASE
    }
    *err = hipGetLastError();
    return true;
}

hipError_t launch_augment_boxes(const dal3_augment_boxes_args* a, hipStream_t s) {
    if (a->B == 0) return hipSuccess;
    hipLaunchKernelGGL(augment_boxes_kernel, dim3((unsigned)a->B), dim3(AUG_BLOCK), 0, s, *a);
    return hipGetLastError();
}
