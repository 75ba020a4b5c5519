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

#include "dal3_iou_pair.h"

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
