// dal3_iou_pair.h — the geometry of one rotated-box pair (dal3_iou.hip's file comment): IouBox, iou_box, clip_slab,
// box_iou_pair. Included INSIDE an anonymous namespace by dal3_iou.hip and dal3_metrics.hip, each compiled with
// `#pragma clang fp contract(off)` in force before the include, so that every kernel that scores a pair runs the same
// arithmetic and gives the same bits.
#pragma once

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
__device__ __forceinline__ void box_iou_pair(const IouBox<T>& a, const IouBox<T>& b, float& iou_bev, float& iou_3d,
                                             float* clamped_3d = nullptr) {
    // clamped_3d (optional): the reference's boxes_iou3d_gpu, the 3-D intersection over max(union, 1e-6)
    if (a.bad | b.bad) {
        iou_bev = iou_3d = __builtin_nanf("");
        if (clamped_3d) *clamped_3d = iou_3d;
        return;
    }
    const float dx = (float)(a.cx - b.cx), dy = (float)(a.cy - b.cy);
    const float reach = (a.rad + b.rad) * 1.000001f;
    if (dx * dx + dy * dy > reach * reach) {    // bounding circles disjoint
        iou_bev = iou_3d = 0.f;
        if (clamped_3d) *clamped_3d = 0.f;
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
    if (clamped_3d) *clamped_3d = inter3 / fmaxf(u3, 1e-6f);
}
