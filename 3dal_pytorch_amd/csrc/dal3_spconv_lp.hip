// dal3_spconv_lp.hip — the sparse 3-D middle's convolutions on 16-bit MFMA operands (dal3_sp_conv_lp_pack / dal3_sp_conv_lp
// of include/dal3.h): dal3_spconv.hip's output-stationary gather-GEMM on v_mfma_f32_32x32x16_{f16,bf16}, in the same
// orientation: output channels on the MFMA rows, 32 output sites on its columns (= lanes), 16 input channels per k-step.
// Lane (site n, half h) supplies channels 16 s + 8 h + j of k-step s: ONE 16-byte load per k-step from a 16-bit row
// (x16, what the producing layer stored as y16), or two from a float32 row rounded as it is staged (the same values, so
// the same bits); the 1 .. 8 channels of the first layer are scalar loads into one zero-padded k-step. The accumulator
// layout is the fp32 kernel's, and so is its epilogue.
//
// The arithmetic (the contract of include/dal3.h): W' of dal3_fold.h rounded once more, to the 16-bit type, by the packer;
// every gathered activation q(x); products summed in the MFMA's fp32 accumulator FROM ZERO over the present taps in
// ascending order; then b' (float32) is added, then the float32 residual, then ReLU, all in float32. An absent neighbour
// supplies zeros, which change no finite sum, so the bits depend on the site's own row of the table alone.
//
// Weight reuse. At 32 cycles per MFMA a wave holding one tile of 32 sites would need a fresh 1 KiB fragment every 32
// cycles, which L2 cannot feed to every wave. Both remedies are taken: a wave owns T = 2 site tiles (every fragment read
// feeds two MFMAs), and the four waves of a workgroup (256 consecutive sites) share a tap's fragments — all k-steps and
// all out tiles, NKS x MT KiB, in segments of at most 16 KiB — through LDS: the segment after the one in use is fetched into
// registers before the MFMAs of the current one and written to the other half of a double buffer behind them, one barrier
// per segment. A tap that no site of the workgroup has is neither fetched nor run; a tile none of whose sites has the tap
// skips its MFMAs.
#include "dal3_block.h"
#include "dal3_kernels.h"
#include "dal3_lp.h"

namespace {

constexpr int SL_BLOCK = 256, SL_WAVES = 4, SL_T = 2, SL_SITES = SL_WAVES * SL_T * 32;
constexpr int SL_HEAD_BYTES = 256;              // the pack's first section, 64 words: word 0 is its flag

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

__host__ __device__ constexpr int sl_nks(int c_in) { return c_in <= 8 ? 1 : c_in / 16; }     // k-steps of 16 channels

__device__ __forceinline__ int64_t sl_live(const int64_t* n, int64_t cap) {
    if (!n) return cap;
    const int64_t v = *n;
    return v < 0 ? 0 : v > cap ? cap : v;
}

template <class DT>
__device__ __forceinline__ uint16_t sl_round16(float v) {
    return __builtin_bit_cast(uint16_t, (typename DT::elem)v);
}
template <class DT>
__device__ __forceinline__ float sl_widen(uint16_t b) {
    return (float)__builtin_bit_cast(typename DT::elem, b);
}

// the blob: [64 words, word 0 the flag | mt_total * 32 float32 b' | [tap][k-step][out tile][lane][8] 16-bit W']
template <class DT>
__global__ __launch_bounds__(SL_BLOCK) void sp_conv_lp_pack_kernel(const FoldLayer L, int mt_total, int nks, int64_t n_values,
                                                                   int32_t* flag, float* bias, uint16_t* frag, int32_t* status) {
    for (int64_t i = (int64_t)blockIdx.x * SL_BLOCK + threadIdx.x; i < n_values + mt_total * 32; i += (int64_t)gridDim.x * SL_BLOCK) {
        bool bad;
        if (i < mt_total * 32) {
            const int co = (int)i;
            const float v = co < L.c_out ? fold_bias(L, co) : 0.f;
            bias[co] = v;
            bad = bits_nonfinite(v);
        } else {
            const int64_t j = i - mt_total * 32;
            const int e = (int)(j & 7), lane = (int)((j >> 3) & 63);
            const int64_t t = j >> 9;
            const int mt = (int)(t % mt_total), ks = (int)((t / mt_total) % nks), tap = (int)(t / ((int64_t)mt_total * nks));
            const int co = 32 * mt + (lane & 31), ci = 16 * ks + 8 * (lane >> 5) + e;
            float v = 0.f;
            if (co < L.c_out && ci < L.c_in) {
                v = fold_weight(L, ((int64_t)tap * L.c_in + ci) * L.c_out + co, co);
                // W' is a float32 VALUE before it is rounded to 16 bits (two roundings, the contract's)
                asm volatile("" : "+v"(v));
            }
            const uint16_t b = sl_round16<DT>(v);
            frag[j] = b;
            bad = bits_nonfinite(sl_widen<DT>(b));
        }
        if (bad) {
            atomicOr(flag, 1);
            if (status) atomicOr(status, DAL3_SP_BAD_WEIGHT);
        }
    }
}

struct SpLpGeom {
    int taps, c_in, c_out, relu, center;
    int64_t in_cap, out_cap, n_blocks;
    const int64_t* n_out;
    const int32_t* table;
    const float *x, *residual;
    const uint16_t* x16;
    float* y;
    uint16_t* y16;
    const int32_t* flag;
    const float* bias;
    const u32x4_t* frag;
    float* canvas;
    const int32_t* out_idx;
    int32_t cB, cD, cH, cW;
    int32_t* status;
};

// max(v, 0) that keeps a NaN (torch.relu does) and turns -0 into +0
__device__ __forceinline__ float sl_relu(float v) { return v > 0.f ? v : (v == v ? 0.f : v); }

template <class DT>
__device__ __forceinline__ typename DT::v8 sl_pack8(const f32x4& a, const f32x4& b) {
    typename DT::v8 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r[e] = (typename DT::elem)a[e];
        r[4 + e] = (typename DT::elem)b[e];
    }
    return r;
}

// NKS: k-steps of 16 input channels (1 also serves the first layer's 1 .. 8 float32 channels); MT: out tiles of 32 channels
template <class DT, int NKS, int MT>
__global__ __launch_bounds__(SL_BLOCK, 2) void sp_conv_lp_kernel(const SpLpGeom g) {
    typedef typename DT::v8 v8;
    constexpr int FR = NKS * MT;                            // 1 KiB fragments of one tap
    constexpr int NSEG = FR > 16 ? FR / 16 : 1, KSEG = NKS / NSEG;          // a tap is staged in segments of at most 16 KiB
    constexpr int UNITS = FR / NSEG * 64, NU = (UNITS + SL_BLOCK - 1) / SL_BLOCK;     // 16-byte units of a segment, and per thread
    constexpr int KC = KSEG < 4 ? KSEG : 4;                 // k-steps gathered ahead of their MFMAs
    static_assert(KSEG * NSEG == NKS && KSEG % KC == 0, "whole k-steps per segment");
    __shared__ u32x4_t wbuf[2][UNITS];
    __shared__ uint32_t s_mask;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    if (*g.flag) {                              // a folded weight is not finite: the pack is refused
        if (blockIdx.x == 0 && tid == 0) atomicOr(g.status, DAL3_SP_BAD_WEIGHT);
        return;
    }
    const int64_t n_out = sl_live(g.n_out, g.out_cap);
    for (int64_t blk = blockIdx.x; blk < g.n_blocks; blk += gridDim.x) {
        const int64_t base = blk * SL_SITES;
        if (base >= n_out) break;               // (uniform: every thread reads the same count)
        int64_t i[SL_T];
        bool live[SL_T];
#pragma unroll
        for (int j = 0; j < SL_T; ++j) {
            i[j] = base + (wave * SL_T + j) * 32 + n;
            live[j] = i[j] < n_out;
        }
        // the taps that any site of the workgroup has
        if (tid == 0) s_mask = 0u;
        __syncthreads();
        uint32_t mine = 0u;
        for (int tap = 0; tap < g.taps; ++tap) {
            bool any = false;
#pragma unroll
            for (int j = 0; j < SL_T; ++j) {
                const int32_t idx = live[j] ? g.table[(int64_t)tap * g.out_cap + i[j]] : -1;
                any = any || (idx >= 0 && idx < g.in_cap);
            }
            if (__ballot(any) != 0ull) mine |= 1u << tap;
        }
        if (lane == 0 && mine) atomicOr(&s_mask, mine);
        __syncthreads();
        uint32_t rest = s_mask;
        __syncthreads();                        // everyone has read the mask before the next group clears it

        f32x16 acc[MT][SL_T];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int j = 0; j < SL_T; ++j) acc[m][j] = f32x16{};
        }

        if (rest) {
            int tap = __builtin_ctz(rest), seg = 0, cur = 0;
            rest &= rest - 1;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int at = tid + u * SL_BLOCK;
                if (at < UNITS) wbuf[0][at] = g.frag[(int64_t)tap * NSEG * UNITS + at];
            }
            __syncthreads();
            int32_t idx[SL_T];
            bool has[SL_T], any = false;
            while (true) {
                // what is staged behind this segment: the tap's next segment, or the next present tap's first
                int ntap = tap, nseg = seg + 1;
                bool more = true;
                if (nseg == NSEG) {
                    nseg = 0;
                    more = rest != 0u;
                    ntap = more ? __builtin_ctz(rest) : tap;
                }
                u32x4_t st[NU];
                if (more) {
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        const int at = tid + u * SL_BLOCK;
                        if (at < UNITS) st[u] = g.frag[((int64_t)ntap * NSEG + nseg) * UNITS + at];
                    }
                }
                if (seg == 0) {
                    any = false;
#pragma unroll
                    for (int j = 0; j < SL_T; ++j) {
                        idx[j] = live[j] ? g.table[(int64_t)tap * g.out_cap + i[j]] : -1;
                        if (idx[j] >= g.in_cap) idx[j] = -1;
                        has[j] = __ballot(idx[j] >= 0) != 0ull;
                        any = any || has[j];
                    }
                }
                if (any) {
#pragma unroll
                    for (int k0 = 0; k0 < KSEG; k0 += KC) {
                        v8 bv[SL_T][KC];
#pragma unroll
                        for (int j = 0; j < SL_T; ++j) {
                            if (!has[j]) continue;
                            const int64_t row = (int64_t)(idx[j] < 0 ? 0 : idx[j]) * g.c_in;
#pragma unroll
                            for (int kk = 0; kk < KC; ++kk) {
                                const int c0 = 16 * (seg * KSEG + k0 + kk) + 8 * h;
                                u32x4_t w = {0u, 0u, 0u, 0u};
                                if (g.x16) {
                                    if (idx[j] >= 0) w = *reinterpret_cast<const u32x4_t*>(g.x16 + row + c0);
                                    bv[j][kk] = __builtin_bit_cast(v8, w);
                                } else if (NKS == 1 && g.c_in < 16) {
                                    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                                    for (int e = 0; e < 4; ++e) {
                                        if (idx[j] >= 0 && c0 + e < g.c_in) a[e] = g.x[row + c0 + e];
                                        if (idx[j] >= 0 && c0 + 4 + e < g.c_in) b[e] = g.x[row + c0 + 4 + e];
                                    }
                                    bv[j][kk] = sl_pack8<DT>(a, b);
                                } else {
                                    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
                                    if (idx[j] >= 0) {
                                        a = *reinterpret_cast<const f32x4*>(g.x + row + c0);
                                        b = *reinterpret_cast<const f32x4*>(g.x + row + c0 + 4);
                                    }
                                    bv[j][kk] = sl_pack8<DT>(a, b);
                                }
                            }
                        }
#pragma unroll
                        for (int kk = 0; kk < KC; ++kk) {
#pragma unroll
                            for (int m = 0; m < MT; ++m) {
                                const v8 a = __builtin_bit_cast(v8, wbuf[cur][((k0 + kk) * MT + m) * 64 + lane]);
#pragma unroll
                                for (int j = 0; j < SL_T; ++j) {
                                    if (has[j]) acc[m][j] = DT::mfma(a, bv[j][kk], acc[m][j]);
                                }
                            }
                        }
                    }
                }
                if (more) {
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        const int at = tid + u * SL_BLOCK;
                        if (at < UNITS) wbuf[cur ^ 1][at] = st[u];
                    }
                }
                __syncthreads();                // the next segment is staged, and this one's fragments are read
                if (!more) break;
                if (nseg == 0) rest &= rest - 1;
                tap = ntap;
                seg = nseg;
                cur ^= 1;
            }
        }

#pragma unroll
        for (int j = 0; j < SL_T; ++j) {
            if (!live[j]) continue;
            const int64_t r = i[j];
            // a row that is no site (its centre tap is absent: only a bad input row of a submanifold layer) is +0
            const bool zero = g.center >= 0 && g.table[(int64_t)g.center * g.out_cap + r] < 0;
            int32_t cb = 0, cz = 0, cy = 0, cx = 0;
            bool on_canvas = false;
            if (g.canvas) {
                cb = g.out_idx[4 * r], cz = g.out_idx[4 * r + 1], cy = g.out_idx[4 * r + 2], cx = g.out_idx[4 * r + 3];
                on_canvas = cb >= 0 && cb < g.cB && cz >= 0 && cz < g.cD && cy >= 0 && cy < g.cH && cx >= 0 && cx < g.cW;
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c0 = 32 * m + 8 * q + 4 * h;     // registers 4q .. 4q + 3: four consecutive channels
                    if (c0 >= g.c_out) continue;
                    f32x4 v = f32x4{acc[m][j][4 * q], acc[m][j][4 * q + 1], acc[m][j][4 * q + 2], acc[m][j][4 * q + 3]};
                    v += *reinterpret_cast<const f32x4*>(g.bias + c0);
                    if (g.residual) v += *reinterpret_cast<const f32x4*>(g.residual + r * g.c_out + c0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (g.relu) v[e] = sl_relu(v[e]);
                        if (zero) v[e] = 0.f;
                    }
                    if (g.y) *reinterpret_cast<f32x4*>(g.y + r * g.c_out + c0) = v;
                    if (g.y16) {
                        u32x2_t p;
                        p[0] = (uint32_t)sl_round16<DT>(v[0]) | ((uint32_t)sl_round16<DT>(v[1]) << 16);
                        p[1] = (uint32_t)sl_round16<DT>(v[2]) | ((uint32_t)sl_round16<DT>(v[3]) << 16);
                        *reinterpret_cast<u32x2_t*>(g.y16 + r * g.c_out + c0) = p;
                    }
                    if (on_canvas) {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            g.canvas[((((int64_t)cb * g.c_out + c0 + e) * g.cD + cz) * g.cH + cy) * g.cW + cx] = v[e];
                    }
                }
            }
        }
    }
}

template <class DT, int NKS>
void sl_launch_mt(const SpLpGeom& g, int mt, dim3 grid, hipStream_t s) {
    if (mt == 4) hipLaunchKernelGGL((sp_conv_lp_kernel<DT, NKS, 4>), grid, dim3(SL_BLOCK), 0, s, g);
    else if (mt == 2) hipLaunchKernelGGL((sp_conv_lp_kernel<DT, NKS, 2>), grid, dim3(SL_BLOCK), 0, s, g);
    else hipLaunchKernelGGL((sp_conv_lp_kernel<DT, NKS, 1>), grid, dim3(SL_BLOCK), 0, s, g);
}

template <class DT>
void sl_launch(const SpLpGeom& g, int nks, int mt, dim3 grid, hipStream_t s) {
    switch (nks) {
        case 1: sl_launch_mt<DT, 1>(g, mt, grid, s); break;
        case 2: sl_launch_mt<DT, 2>(g, mt, grid, s); break;
        case 4: sl_launch_mt<DT, 4>(g, mt, grid, s); break;
        default: sl_launch_mt<DT, 8>(g, mt, grid, s); break;
    }
}

}  // namespace

size_t sp_conv_lp_pack_bytes(int taps, int c_in, int c_out) {
    const int64_t mt = (c_out + 31) / 32, nks = sl_nks(c_in);
    return (size_t)(SL_HEAD_BYTES + mt * 32 * 4 + (int64_t)taps * nks * mt * 1024);
}

hipError_t launch_sp_conv_lp_pack(const FoldLayer& L, int taps, int dtype, void* out, int32_t* status, hipStream_t s) {
    const int mt = (L.c_out + 31) / 32, nks = sl_nks(L.c_in);
    const int64_t n_values = (int64_t)taps * nks * mt * 512, total = n_values + mt * 32;
    const hipError_t e = launch_fill_words(out, SL_HEAD_BYTES / 4, 0, s);
    if (e != hipSuccess) return e;
    int32_t* flag = static_cast<int32_t*>(out);
    float* bias = reinterpret_cast<float*>(static_cast<char*>(out) + SL_HEAD_BYTES);
    uint16_t* frag = reinterpret_cast<uint16_t*>(bias + mt * 32);
    const dim3 grid(grid_clamp((total + SL_BLOCK - 1) / SL_BLOCK, 4096, 0));
    if (dtype == DAL3_F16)
        hipLaunchKernelGGL(sp_conv_lp_pack_kernel<FP16>, grid, dim3(SL_BLOCK), 0, s, L, mt, nks, n_values, flag, bias, frag, status);
    else
        hipLaunchKernelGGL(sp_conv_lp_pack_kernel<BF16>, grid, dim3(SL_BLOCK), 0, s, L, mt, nks, n_values, flag, bias, frag, status);
    return hipGetLastError();
}

hipError_t launch_sp_conv_lp(const dal3_sp_conv_lp_args* args, hipStream_t s) {
    const dal3_sp_conv_lp_args& a = *args;
    if (a.canvas) {
        const hipError_t e = launch_fill_words(
            a.canvas, (size_t)(a.canvas_B * a.c_out * a.canvas_shape[0] * a.canvas_shape[1] * a.canvas_shape[2]), 0, s);
        if (e != hipSuccess) return e;
    }
    if (a.out_capacity <= 0) return hipSuccess;
    SpLpGeom g = {};
    g.taps = a.taps, g.c_in = a.c_in, g.c_out = a.c_out, g.relu = a.relu, g.center = a.center_tap;
    const int mt = (a.c_out + 31) / 32, nks = sl_nks(a.c_in);
    g.in_cap = a.in_capacity, g.out_cap = a.out_capacity;
    g.n_blocks = (a.out_capacity + SL_SITES - 1) / SL_SITES;
    g.n_out = a.n_out, g.table = a.table, g.x = a.x, g.residual = a.residual, g.y = a.y;
    g.x16 = static_cast<const uint16_t*>(a.x16), g.y16 = static_cast<uint16_t*>(a.y16);
    const char* blob = static_cast<const char*>(a.packed);
    g.flag = reinterpret_cast<const int32_t*>(blob);
    g.bias = reinterpret_cast<const float*>(blob + SL_HEAD_BYTES);
    g.frag = reinterpret_cast<const u32x4_t*>(blob + SL_HEAD_BYTES + mt * 32 * 4);
    g.canvas = a.canvas, g.out_idx = a.out_indices;
    g.cB = (int32_t)a.canvas_B, g.cD = a.canvas_shape[0], g.cH = a.canvas_shape[1], g.cW = a.canvas_shape[2];
    g.status = a.status;
    const dim3 grid(grid_clamp(g.n_blocks, 65535 * 16, a.max_workgroups));
    if (a.dtype == DAL3_F16) sl_launch<FP16>(g, nks, mt, grid, s);
    else sl_launch<BF16>(g, nks, mt, grid, s);
    return hipGetLastError();
}
