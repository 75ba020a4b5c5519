// dal3_geom.h — the reference's points-in-rotated-box test on the device.
// det3d/core/bbox/box_np_ops.py:641-647 (points_in_rbbox) -> det3d/core/bbox/geometry.py:240-275
// (_points_in_convex_polygon_3d_jit): a point is OUTSIDE as soon as one of the six faces gives
//     ((px*nx + py*ny) + pz*nz) + d >= 0
// evaluated left to right with every product and sum rounded on its own (NumPy scalar arithmetic / numba without
// fastmath): no FMA contraction here either — face_sign() below, under `#pragma clang fp contract(off)`. (HIP's
// __fmul_rn / __fadd_rn are plain `*` and `+`: inlined into an expression they are contracted like any other under
// hipcc's default -ffp-contract=fast-honor-pragmas, and a fused x*nx + y*ny moves points lying within a few ulps of a
// rotated face to the other side of it: tests/test_gpu_crops_routes.py, case "faces".) A NaN never compares >= 0, so a
// NaN point stays inside — kept. The face equations [nx,ny,nz,d] come from the host (O(#boxes) NumPy, the same
// calls the reference makes: sin/cos of a float32 yaw are NumPy's own SIMD routines and cannot be reproduced bit
// for bit by device libm); they are stored as float64. The expression is evaluated in float32 when points AND
// boxes are float32 (the sweep / detector case), otherwise in float64 (the Datasets: float64 points, float32 box).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DAL3_PLANE_DOUBLES 24            // 6 faces x [nx, ny, nz, d]

// `v >= 0` on the bit pattern: the reference's NaN behaviour is part of the contract here (a NaN point is inside
// every box), so the compare is done in integers and does not depend on the floating-point flags of the build
// (only dal3_pointmlp*.hip are compiled with -fno-honor-nans; this header's users keep IEEE NaN semantics).
__device__ __forceinline__ bool ge_zero(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x7fffffffu) <= 0x7f800000u && ((b >> 31) == 0 || (b << 1) == 0);
}
__device__ __forceinline__ bool ge_zero(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b & 0x7fffffffffffffffull) <= 0x7ff0000000000000ull && ((b >> 63) == 0 || (b << 1) == 0);
}

template <typename T>
__device__ __forceinline__ T face_sign(T x, T y, T z, T nx, T ny, T nz, T d) {
#pragma clang fp contract(off)
    const T a = x * nx, b = y * ny, c = z * nz;
    const T ab = a + b;
    const T abc = ab + c;
    return abc + d;
}

__device__ __forceinline__ bool inside_box_f32(const double* __restrict__ pl, float x, float y, float z) {
    bool in = true;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const float nx = (float)pl[f * 4 + 0], ny = (float)pl[f * 4 + 1], nz = (float)pl[f * 4 + 2], d = (float)pl[f * 4 + 3];
        const float sgn = face_sign(x, y, z, nx, ny, nz, d);
        in = in && !ge_zero(sgn);
    }
    return in;
}

__device__ __forceinline__ bool inside_box_f64(const double* __restrict__ pl, double x, double y, double z) {
    bool in = true;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const double sgn = face_sign(x, y, z, pl[f * 4 + 0], pl[f * 4 + 1], pl[f * 4 + 2], pl[f * 4 + 3]);
        in = in && !ge_zero(sgn);
    }
    return in;
}
