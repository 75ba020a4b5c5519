// dal3_sweeps.hip — dal3_sweep_merge (include/dal3.h): the Waymo branch of LoadPointCloudFromFile
// (det3d/datasets/pipelines/loading.py:61-91, 140-168) for a whole batch in one launch. A sample's current frame and its
// earlier sweeps lie in the raw arena as they came off the disk, xyz (n, 3) and feature (n, 2) in planes of their own; the
// kernel writes the merged rows [x, y, z, tanh(feature0), feature1 (, time)] the voxeliser reads, and the batch's
// point_offsets.
//
// A streaming kernel: one output row per lane per step of a grid-stride loop, so a wave's 64 rows are 768 contiguous
// bytes of the xyz plane, 512 of the feature plane (one 8-byte load per lane where the plane is 8-byte aligned) and 1536
// (1280 without the time column) of the output (8-byte stores where the output is: a six-column row is 24 bytes). The
// segment of a row is the last entry of the table whose first output row is <= the row: a binary search over
// B * nsweeps entries that neighbouring lanes resolve alike. Every output row is written once, by the one lane that owns
// it; there is no atomic and nothing is read back.
//
// Arithmetic, the same for every grid: the transform is ((m0 x + m1 y) + m2 z) + m3 per row of the matrix in float64,
// each product and sum rounded on its own (no fused multiply-add), cast once; the intensity is the float64 tanh of the
// float32 value, cast once. NaN and infinities go through both as IEEE-754 has them.
#include "dal3_block.h"
#include "dal3_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int SWEEP_BLOCK = 256;

__device__ __forceinline__ float transform_row(const double* m, double x, double y, double z) {
    return (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], x), __dmul_rn(m[1], y)), __dmul_rn(m[2], z)), m[3]);
}

template <int C>
__global__ __launch_bounds__(SWEEP_BLOCK) void sweep_merge_kernel(const dal3_sweep_segment* __restrict__ seg, int64_t B,
                                                                   int nsweeps, int64_t N, float* __restrict__ out,
                                                                   int64_t* __restrict__ point_offsets) {
    const int64_t stride = (int64_t)gridDim.x * SWEEP_BLOCK, first = (int64_t)blockIdx.x * SWEEP_BLOCK + threadIdx.x;
    const int64_t S = B * nsweeps;
    const bool out8 = (reinterpret_cast<uintptr_t>(out) & 7) == 0;
    for (int64_t r = first; r < N; r += stride) {
        // the segment of row r: the last s with out_row[s] <= r (an empty segment shares its out_row with the next one)
        int64_t lo = 0, hi = S;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (seg[mid].out_row <= r) lo = mid;
            else hi = mid;
        }
        const dal3_sweep_segment& g = seg[lo];
        const int64_t i = r - g.out_row;
        if (i < 0 || i >= g.n) continue;        // a row of no segment: only a table that is no partition of [0, N)
        const float* p = g.xyz + 3 * i;
        float x = p[0], y = p[1], z = p[2];
        float f0, f1;
        if ((reinterpret_cast<uintptr_t>(g.feature) & 7) == 0) {
            const float2 f = reinterpret_cast<const float2*>(g.feature)[i];
            f0 = f.x, f1 = f.y;
        } else {
            f0 = g.feature[2 * i], f1 = g.feature[2 * i + 1];
        }
        if (g.has_transform) {
            const double dx = (double)x, dy = (double)y, dz = (double)z;
            x = transform_row(g.matrix, dx, dy, dz);
            y = transform_row(g.matrix + 4, dx, dy, dz);
            z = transform_row(g.matrix + 8, dx, dy, dz);
        }
        const float t = (float)tanh((double)f0);
        float* o = out + r * C;
        if (C == 6 && out8) {
            float2* o2 = reinterpret_cast<float2*>(o);
            o2[0] = make_float2(x, y);
            o2[1] = make_float2(z, t);
            o2[2] = make_float2(f1, g.time);
        } else {
            o[0] = x, o[1] = y, o[2] = z, o[3] = t, o[4] = f1;
            if (C == 6) o[5] = g.time;
        }
    }
    // sample b starts where its current frame does; the batch ends at N
    for (int64_t b = first; b <= B; b += stride) point_offsets[b] = b == B ? N : seg[b * nsweeps].out_row;
}

}  // namespace

hipError_t launch_sweep_merge(const dal3_sweep_segment* segments, int64_t B, int nsweeps, int64_t N, float* out,
                              int64_t* point_offsets, int64_t max_workgroups, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    const int64_t work = N > B + 1 ? N : B + 1;
    const dim3 grid(grid_clamp((work + SWEEP_BLOCK - 1) / SWEEP_BLOCK, 2048, max_workgroups)), blk(SWEEP_BLOCK);
    if (nsweeps > 1) hipLaunchKernelGGL(sweep_merge_kernel<6>, grid, blk, 0, s, segments, B, nsweeps, N, out, point_offsets);
    else hipLaunchKernelGGL(sweep_merge_kernel<5>, grid, blk, 0, s, segments, B, nsweeps, N, out, point_offsets);
    return hipGetLastError();
}
