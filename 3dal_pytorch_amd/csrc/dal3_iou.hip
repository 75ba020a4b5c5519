// dal3_iou.hip — rotated-box IoU (bird's-eye view and 3D) of [x, y, z, l, w, h, yaw] boxes: the quantity of the
// reference's det3d/ops/iou3d_nms boxes_iou_bev / boxes_iou3d_gpu, by a different construction.
//
// Geometry of one pair (a, b), shared by both kernels (box_iou_pair), so that pairwise[i, j] and paired(a[i], b[j])
// are the same bits:
//   - a's centre is taken relative to b's in the input precision, then rotated into b's frame; a's rotation in that
//     frame is the single angle yaw_a - yaw_b. The result is translation-invariant and equal yaws give an exactly
//     axis-aligned clip.
//   - a's four corners are clipped against the slab |x| <= l_b/2, then the slab |y| <= w_b/2 (Sutherland–Hodgman one
//     slab at a time), and the area is the shoelace sum of what is left.
//   - A clip step turns every edge into exactly two points: the ends of the part of the edge inside the slab, or, for
//     an edge wholly outside, its two ends projected onto the slab's side. Every extra point lies on the side line
//     between an exit and the next entry, collinear with them, and adds nothing to the shoelace sum. So the polygon
//     lives in fixed arrays (4 -> 8 -> 16 points) indexed only by unrolled constants: no compaction, no runtime
//     index, no scratch (check: .private_segment_fixed_size 0 in the code object, tests/test_iou_cpu.py).
// Pairs whose bounding circles are disjoint are exactly 0 before any of that. A non-finite input gives NaN for its
// pairs; a union <= 0 (degenerate boxes) gives 0; negative sizes count as 0.
#include "dal3_kernels.h"

// no FMA contraction in this file: the pairwise and paired kernels inline the same arithmetic into different code, and
// a contraction the backend forms in one and not in the other would break their bit-identity
#pragma clang fp contract(off)

namespace {

constexpr int IOU_TB = 64;                      // b boxes per pairwise tile: one per lane of a wave64
constexpr int IOU_TA = 16;                      // a boxes per pairwise tile: four per wave
constexpr int IOU_BLOCK = 256;

template <typename T>
struct IouBox {
    T cx, cy, cz, yaw;                          // input precision: the differences between two boxes are taken in it
    float hl, hw, hh;                           // half extents
    float c, s;                                 // cos / sin of yaw (rotates a world offset into this box's frame)
    float area, vol, rad;                       // l w, l w h, radius of the BEV rectangle's circumcircle
    int bad;                                    // a non-finite input
};

__device__ __forceinline__ void sin_cos(float x, float* s, float* c) { sincosf(x, s, c); }
__device__ __forceinline__ void sin_cos(double x, double* s, double* c) { sincos(x, s, c); }

template <typename T>
__device__ __forceinline__ IouBox<T> iou_box(const T* p) {
    IouBox<T> q;
    q.cx = p[0];
    q.cy = p[1];
    q.cz = p[2];
    q.yaw = p[6];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) finite = finite && isfinite(p[k]);
    q.bad = finite ? 0 : 1;
    const float l = fmaxf((float)p[3], 0.f), w = fmaxf((float)p[4], 0.f), h = fmaxf((float)p[5], 0.f);
    q.hl = 0.5f * l;
    q.hw = 0.5f * w;
    q.hh = 0.5f * h;
    T s, c;
    sin_cos(q.yaw, &s, &c);
    q.c = (float)c;
    q.s = (float)s;
    q.area = l * w;
    q.vol = q.area * h;
    q.rad = sqrtf(q.hl * q.hl + q.hw * q.hw);
    return q;
}

// One slab clip |u| <= H of an N-point convex polygon (u, v) -> 2N points, see the file comment.
template <int N>
__device__ __forceinline__ void clip_slab(const float (&u)[N], const float (&v)[N], float H, float (&uo)[2 * N],
                                          float (&vo)[2 * N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int k1 = (k + 1) % N;
        const float pu = u[k], pv = v[k], qu = u[k1], qv = v[k1];
        const float du = qu - pu, dv = qv - pv;
        float t0 = 0.f, t1 = 1.f;
        if (du != 0.f) {
            const float r = 1.f / du;
            const float ta = (-H - pu) * r, tb = (H - pu) * r;
            t0 = fmaxf(0.f, fminf(ta, tb));
            t1 = fminf(1.f, fmaxf(ta, tb));
        } else if (fabsf(pu) > H) {
            t0 = 1.f;                           // parallel to the slab and outside it: empty
            t1 = 0.f;
        }
        if (!(t0 <= t1)) {                      // wholly outside: both ends, projected onto the side below
            t0 = 0.f;
            t1 = 1.f;
        }
        const float su = t0 == 0.f ? pu : pu + t0 * du, sv = t0 == 0.f ? pv : pv + t0 * dv;
        const float eu = t1 == 1.f ? qu : pu + t1 * du, ev = t1 == 1.f ? qv : pv + t1 * dv;
        uo[2 * k] = fminf(fmaxf(su, -H), H);
        vo[2 * k] = sv;
        uo[2 * k + 1] = fminf(fmaxf(eu, -H), H);
        vo[2 * k + 1] = ev;
    }
}

template <typename T>
__device__ __forceinline__ void box_iou_pair(const IouBox<T>& a, const IouBox<T>& b, float& iou_bev, float& iou_3d) {
    if (a.bad | b.bad) {
        iou_bev = iou_3d = __builtin_nanf("");
        return;
    }
    const float dx = (float)(a.cx - b.cx), dy = (float)(a.cy - b.cy);
    const float reach = (a.rad + b.rad) * 1.000001f;
    if (dx * dx + dy * dy > reach * reach) {    // bounding circles disjoint
        iou_bev = iou_3d = 0.f;
        return;
    }
    // a in b's frame: centre, then the half-length and half-width axes rotated by yaw_a - yaw_b
    const float px = b.c * dx + b.s * dy, py = b.c * dy - b.s * dx;
    float sr, cr;
    sincosf((float)(a.yaw - b.yaw), &sr, &cr);
    const float ux = cr * a.hl, uy = sr * a.hl, vx = -(sr * a.hw), vy = cr * a.hw;
    const float x4[4] = {px + ux + vx, px - ux + vx, px - ux - vx, px + ux - vx};   // counter-clockwise
    const float y4[4] = {py + uy + vy, py - uy + vy, py - uy - vy, py + uy - vy};
    float x8[8], y8[8], y16[16], x16[16];
    clip_slab<4>(x4, y4, b.hl, x8, y8);
    clip_slab<8>(y8, x8, b.hw, y16, x16);
    float twice = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) twice += x16[k] * y16[(k + 1) % 16] - x16[(k + 1) % 16] * y16[k];
    const float inter = fminf(fmaxf(0.5f * twice, 0.f), fminf(a.area, b.area));
    const float u2 = a.area + b.area - inter;
    iou_bev = u2 > 0.f ? inter / u2 : 0.f;
    // z overlap in b's frame (translation-invariant like the rest)
    const float dz = (float)(a.cz - b.cz);
    const float zo = fmaxf(fminf(dz + a.hh, b.hh) - fmaxf(dz - a.hh, -b.hh), 0.f);
    const float inter3 = inter * zo, u3 = a.vol + b.vol - inter3;
    iou_3d = u3 > 0.f ? inter3 / u3 : 0.f;
}

// (n, m): one tile = IOU_TA rows of a x IOU_TB columns of b, both derived once into LDS; lane = column, so a wave
// stores 64 consecutive floats of one row. Blocks are numbered row-tile-major, column tile fastest.
template <typename T>
__global__ __launch_bounds__(IOU_BLOCK) void box_iou_pairwise_kernel(const T* __restrict__ a, int64_t n,
                                                                     const T* __restrict__ b, int64_t m, int64_t tiles_m,
                                                                     float* __restrict__ out_bev,
                                                                     float* __restrict__ out_3d) {
    __shared__ IouBox<T> sb[IOU_TB];
    __shared__ IouBox<T> sa[IOU_TA];
    const int64_t tile = blockIdx.x;
    const int64_t ti = tile / tiles_m, tj = tile - ti * tiles_m;
    const int64_t i0 = ti * IOU_TA, j0 = tj * IOU_TB;
    const int t = threadIdx.x;
    if (t < IOU_TB) {
        if (j0 + t < m) sb[t] = iou_box(b + (j0 + t) * 7);
    } else if (t < IOU_TB + IOU_TA) {
        const int r = t - IOU_TB;
        if (i0 + r < n) sa[r] = iou_box(a + (i0 + r) * 7);
    }
    __syncthreads();
    const int lane = t & 63, wave = t >> 6;
    const int64_t j = j0 + lane;
    if (j >= m) return;                         // no barrier below
    const IouBox<T> bj = sb[lane];
#pragma unroll
    for (int k = 0; k < IOU_TA / 4; ++k) {
        const int r = wave + 4 * k;
        const int64_t i = i0 + r;
        if (i >= n) break;
        float vb, v3;
        box_iou_pair(sa[r], bj, vb, v3);
        if (out_bev) out_bev[i * m + j] = vb;
        if (out_3d) out_3d[i * m + j] = v3;
    }
}

template <typename T>
__global__ __launch_bounds__(IOU_BLOCK) void box_iou_paired_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                                   int64_t n, float* __restrict__ out_bev,
                                                                   float* __restrict__ out_3d) {
    const int64_t k = (int64_t)blockIdx.x * IOU_BLOCK + threadIdx.x;
    if (k >= n) return;
    float vb, v3;
    box_iou_pair(iou_box(a + k * 7), iou_box(b + k * 7), vb, v3);
    if (out_bev) out_bev[k] = vb;
    if (out_3d) out_3d[k] = v3;
}

}  // namespace

int64_t box_iou_pairwise_blocks(int64_t n, int64_t m) {
    return ((n + IOU_TA - 1) / IOU_TA) * ((m + IOU_TB - 1) / IOU_TB);
}
int64_t box_iou_paired_blocks(int64_t n) { return (n + IOU_BLOCK - 1) / IOU_BLOCK; }

hipError_t launch_box_iou_pairwise(const void* a, int64_t n, const void* b, int64_t m, int boxes_f64, float* iou_bev,
                                   float* iou_3d, hipStream_t s) {
    if (n <= 0 || m <= 0) return hipSuccess;
    const dim3 grid((unsigned)box_iou_pairwise_blocks(n, m));
    const int64_t tiles_m = (m + IOU_TB - 1) / IOU_TB;
    if (boxes_f64)
        hipLaunchKernelGGL(box_iou_pairwise_kernel<double>, grid, dim3(IOU_BLOCK), 0, s, (const double*)a, n,
                           (const double*)b, m, tiles_m, iou_bev, iou_3d);
    else
        hipLaunchKernelGGL(box_iou_pairwise_kernel<float>, grid, dim3(IOU_BLOCK), 0, s, (const float*)a, n,
                           (const float*)b, m, tiles_m, iou_bev, iou_3d);
    return hipGetLastError();
}

hipError_t launch_box_iou_paired(const void* a, const void* b, int64_t n, int boxes_f64, float* iou_bev, float* iou_3d,
                                 hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)box_iou_paired_blocks(n));
    if (boxes_f64)
        hipLaunchKernelGGL(box_iou_paired_kernel<double>, grid, dim3(IOU_BLOCK), 0, s, (const double*)a,
                           (const double*)b, n, iou_bev, iou_3d);
    else
        hipLaunchKernelGGL(box_iou_paired_kernel<float>, grid, dim3(IOU_BLOCK), 0, s, (const float*)a,
                           (const float*)b, n, iou_bev, iou_3d);
    return hipGetLastError();
}
